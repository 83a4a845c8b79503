"""websocketframeBatchControlRepliesDevice (libwsframe_amd_reply.so) on the GPU against the
sequential model (reply_oracle.py) and the hand-written directed table (reply_cases.py). Every
call compares d_tx byte for byte (a 0xEE fill must be intact past min(total, capacity)), d_tx_off,
d_reply_res and d_reply_state, and the bytes of d_buf, d_desc, d_res and d_proto_res, which must
come back unchanged."""
import ctypes as C

import numpy as np
import pytest

import high_arena as H
import proto_cases as PC
import proto_oracle as P
import reply_cases as RC
import reply_oracle as R
from util_amd import _lib
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_lib.load_reply_lib()                                        # a missing library fails here, it never skips

FILL = R.FILL
WM, LAST = R.WIRE_MASKED, R.LAST_PING_ONLY
SLACK = 48


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)


def i64(dev, a):
    return torch.from_numpy(np.asarray(a, np.uint64).astype(np.int64)).to(dev)


def i32(dev, a):
    return None if a is None else torch.from_numpy(np.asarray(a, np.uint32).astype(np.int32)).to(dev)


def check_call(dev, d_buf, d_so, d_desc, d_res, nseg, mf, flags, proto, fail, keys, state, expect, tag, cap=None, window=None):
    """one call on device tensors; proto: PROTO_RES records or None; fail / keys / state: numpy u32
    or None (NULL); expect: (tx, tx_off, res, state) of the model. Returns the state words out."""
    etx, eoff, eres, est = expect
    total = len(etx)
    cap = total + 16 if cap is None else cap
    tx_t = torch.full((max(total, cap) + SLACK,), FILL, dtype=torch.uint8, device=dev)
    off_t = torch.full((nseg + 1,), 0x6E6E6E6E6E6E6E6E, dtype=torch.int64, device=dev)
    res_t = torch.full((max(1, nseg) * 16,), FILL, dtype=torch.uint8, device=dev)
    pr_t = None if proto is None else up(dev, proto)
    st_t = i32(dev, state)
    seen = d_buf if window is None else d_buf[window[0]:window[1]]
    held = [t for t in (seen, d_desc, d_res, pr_t) if t is not None]
    before = [t.clone() for t in held]
    W.batch_control_replies_device(d_buf, d_so, d_desc, d_res, mf, tx_t, off_t, res_t, flags, pr_t, i32(dev, fail), i32(dev, keys),
                                   st_t, tx_capacity=cap)
    torch.cuda.synchronize()
    for t, b in zip(held, before):
        assert torch.equal(t, b), "%s: an input was modified" % tag
    goff = off_t.cpu().numpy().view(np.uint64)
    bad = np.nonzero(goff != eoff)[0]
    assert not len(bad), "%s: d_tx_off[%d] = %d, model %d" % (tag, bad[0], goff[bad[0]], eoff[bad[0]])
    gres = res_t.cpu().numpy().view(R.RES_DTYPE)[:nseg]
    bad = np.nonzero(gres != eres)[0]
    assert not len(bad), "%s: segment %d result %s, model %s" % (tag, bad[0], gres[bad[0]], eres[bad[0]])
    g = tx_t.cpu().numpy()
    fit = min(total, cap)
    want = np.frombuffer(etx, np.uint8)[:fit]
    bad = np.nonzero(g[:fit] != want)[0]
    if len(bad):
        s = int(np.searchsorted(eoff, bad[0], side="right")) - 1
        raise AssertionError("%s: tx byte %d (segment %d + %d) is %#x, model %#x (%d bytes differ)" % (
            tag, bad[0], s, bad[0] - int(eoff[s]), g[bad[0]], want[bad[0]], len(bad)))
    assert (g[fit:] == FILL).all(), "%s: bytes written past min(total, capacity) = %d" % (tag, fit)
    if state is None:
        return None
    gw = st_t.cpu().numpy().view(np.uint32)
    bad = np.nonzero(gw != est)[0]
    assert not len(bad), "%s: segment %d state %x -> %x, model %x" % (tag, bad[0], state[bad[0]], gw[bad[0]], est[bad[0]])
    return gw


def run_case(dev, c, tag="", flags=None, state="own", cap=None, expect=None):
    """a Case's oracle descriptors on the device, the wire as the flags say"""
    flags = c.flags if flags is None else flags
    st = c.state if isinstance(state, str) else state
    exp = c.expect(flags, st) if expect is None else expect
    b = c.b
    return check_call(dev, up(dev, c.wire(flags)), i64(dev, b.seg_off), up(dev, b.desc), up(dev, b.res), b.nseg, b.max_frames,
                      flags, c.proto, c.fail, c.keys, st, exp, tag, cap)


# ------------------------------------------------------------------ 1: the table, behind every feeder

def device_batch(dev, b):
    n = b.nseg * b.max_frames
    return dict(d=up(dev, b.raw), so=i64(dev, b.seg_off), sl=i64(dev, b.seg_len),
                desc=torch.zeros(32 * n, dtype=torch.uint8, device=dev), res=torch.zeros(16 * b.nseg, dtype=torch.uint8, device=dev),
                out=torch.zeros(len(b.raw) + 64, dtype=torch.uint8, device=dev),
                msg=torch.zeros(32 * n, dtype=torch.uint8, device=dev), nmsg=torch.zeros(b.nseg, dtype=torch.int32, device=dev))


def feed(dev, b, feeder):
    """run a decode entry point on the Batch; returns (d_buf, d_desc, d_res, flag that goes with it)"""
    t = device_batch(dev, b)
    if feeder == "decode":
        W.batch_decode_device(t["d"], t["so"], t["sl"], b.max_frames, t["desc"], t["res"])
        return t["d"], t["desc"], t["res"], 0
    flags = W.REASM_CONTROL_DIRECT if feeder == "ctl" else 0
    W.batch_reassemble_device(t["d"], t["so"], t["sl"], b.max_frames, t["desc"], t["res"], t["out"], t["msg"], t["nmsg"],
                              flags=flags, readcache_max=(1 << 30) if feeder == "ex" else 0)
    return t["d"], t["desc"], t["res"], WM


@pytest.mark.parametrize("feeder", ["oracle", "oracle wire-masked", "decode", "reasm", "ex", "ctl"])
def test_directed_table(dev, feeder):
    """every row against the reply bytes written by hand in the table; descriptors from the decode
    oracle (both wires), from the in-place decode and from the three reassembly calls (the wire
    still masked: WIRE_MASKED). The rows whose last frame is counted but not consumed need the
    oracle's descriptors: no feeder reports such a frame for a complete wire."""
    for rows in RC.table_groups():
        if not feeder.startswith("oracle"):
            rows = [r for r in rows if not r["unconsume"]]
        tag = "table %s flags %d keyed %d" % (feeder, rows[0]["flags"], rows[0]["keyed"])
        exp = RC.table_expect(rows)
        if feeder.startswith("oracle"):
            run_case(dev, RC.table_case(rows, WM if "masked" in feeder else 0), tag, expect=exp)
            continue
        c = RC.table_case(rows)
        d_buf, d_desc, d_res, wm = feed(dev, c.b, feeder)
        check_call(dev, d_buf, i64(dev, c.b.seg_off), d_desc, d_res, c.b.nseg, c.b.max_frames, c.flags | wm, c.proto, c.fail,
                   c.keys, c.state, exp, tag)


def short_script():
    f, p = PC.frame, PC.PING
    return [f(p, b"a"), f(PC.TEXT, b"t"), f(p, b"bcd"), f(p, bytes(range(125))), PC.close(1001, b"bye"), f(p, b"late"),
            PC.close(1000), f(PC.BIN, b"z")]


def test_feeder_stream_decode(dev):
    """one raw stream: descriptors from websocketframeStreamDecodeDevice, one segment at offset 0"""
    frames = PC.quiet(300) + short_script()[:4] + PC.quiet(290) + short_script()[4:]
    b = PC.Batch([frames], len(frames) + 3)
    d = up(dev, b.raw)
    desc = torch.zeros(32 * b.max_frames, dtype=torch.uint8, device=dev)
    res = torch.zeros(16, dtype=torch.uint8, device=dev)
    W.stream_decode_device(d, b.seg_len[0], b.max_frames, desc, res)
    c = RC.Case(b, 0, None, None, None, np.zeros(1, np.uint32))
    exp = c.expect()
    pings = sum(1 for f in frames[:304 + 290] if f[0] == 0x89 and f[1] & 0x7F <= 125)       # (the CLOSE is frame 594)
    assert pings > 50 and tuple(exp[2][0])[:3] == (pings, R.CLOSE_ECHO, 1001) and exp[3][0] == R.ST_CLOSE_SENT
    check_call(dev, d, i64(dev, [0]), desc, res, 1, b.max_frames, 0, None, None, None, c.state, exp, "stream")


# ------------------------------------------------------------------ 2: body lengths and alignments

LENS = [0, 1, 2, 3, 4, 7, 8, 15, 16, 17, 124, 125]


def alignment_batch(masked):
    """per body length and source alignment 0..15 one segment [ping of p bytes, ping of the
    length]: p (0..15) is chosen so that the second body starts at the alignment, and its PONG of
    2 + p bytes shifts the destination. Then the pings that are not answered: 126 bytes, without
    FIN, counted but not consumed."""
    rng = np.random.default_rng(125)
    segs, pos, want = [], 0, []
    hdr = 6 if masked else 2
    for n in LENS:
        for a in range(16):
            p = (a - (pos + 2 * hdr)) % 16
            seg = [PC.frame(PC.PING, bytes(rng.integers(0, 256, p, dtype=np.uint8)), masked=masked),
                   PC.frame(PC.PING, bytes(rng.integers(0, 256, n, dtype=np.uint8)), masked=masked)]
            want.append((n, a, pos + 2 * hdr + p))
            segs.append(seg)
            pos += sum(len(f) for f in seg)
    segs += [[PC.frame(PC.PING, b"x" * 126, masked=masked)], [PC.frame(PC.PING, b"nofin", fin=0, masked=masked)],
             [PC.frame(PC.PING, b"ok", masked=masked), PC.frame(PC.PING, b"unconsumed", masked=masked)]]
    b = PC.Batch(segs, 2)
    b.unconsume_last(b.nseg - 1, -4)
    for s, (n, a, off) in enumerate(want):
        d = b.desc[2 * s + 1]
        assert int(d["datalen"]) == n and (n == 0 or (int(d["data_off"]) == off and off % 16 == a))
    return b


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("keyed", [False, True])
def test_body_lengths_and_alignments(dev, masked, keyed):
    b = alignment_batch(masked)
    keys = np.random.default_rng(9).integers(0, 1 << 32, b.nseg * 3, dtype=np.uint64).astype(np.uint32) if keyed else None
    for flags in (0, WM):
        c = RC.Case(b, flags, None, None, keys, None)
        exp = c.expect()
        assert [int(v) for v in exp[2]["n_pong"][-3:]] == [0, 0, 1] and (exp[2]["n_pong"][:-3] == 2).all()
        run_case(dev, c, "alignments masked %d keyed %d flags %d" % (masked, keyed, flags))


# ------------------------------------------------------------------ 3: tile edges

EDGES = [254, 255, 256, 257, 258, 510, 511, 512, 513, 514]


def list_pos(b, s, k):
    return int(PC.list_starts(b)[s]) + k


@pytest.mark.parametrize("shift", [0, 100])
def test_ping_and_first_close_at_every_tile_edge(dev, shift):
    """a ping with a body of its own, and the first CLOSE, at the list positions 254..258 and
    510..514: each in a segment of 768 frames after `shift` filler frames (as
    tests/test_gpu_proto.py does), the quiet frames around them holding a ping in every seven"""
    segs, at = [PC.quiet(shift)], []
    for i, e in enumerate(EDGES):
        k = e - shift
        segs.append(PC.quiet(k) + [PC.frame(PC.PING, b"edge %d" % e)] + PC.quiet(768 - k - 1))
        segs.append(PC.quiet(k) + [PC.close(1000 + i)] + PC.quiet(766 - k) + [PC.close(3000)])
        at.append(k)
    b = PC.Batch(segs, 768, gap=1)
    assert sorted({list_pos(b, 2 * i + 1, k) % 256 for i, k in enumerate(at)}) == [0, 1, 2, 254, 255]
    for flags in (0, LAST):
        c = RC.Case(b, flags, None, None, None, np.zeros(b.nseg, np.uint32))
        exp = c.expect()
        assert [int(v) for v in exp[2]["close_status"][2::2]] == [1000 + i for i in range(len(EDGES))]
        run_case(dev, c, "edges shift %d flags %d" % (shift, flags))


def test_pings_span_three_tiles_close_in_the_last(dev):
    frames = [PC.frame(PC.PING, bytes([k & 0xFF]) * (k % 9)) for k in range(700)]
    frames[690] = PC.close(1001)
    b = PC.Batch([PC.quiet(37), frames, PC.quiet(5)], 700)
    for flags in (0, LAST):
        c = RC.Case(b, flags, None, None, None, None)
        exp = c.expect()
        assert tuple(exp[2][1])[:3] == (1 if flags else 690, R.CLOSE_ECHO, 1001)
        run_case(dev, c, "three tiles flags %d" % flags)
    c = RC.Case(b, 0, [(R.NONE, 0), (600, 1009), (R.NONE, 0)], None, None, None)
    assert tuple(c.expect()[2][1])[:3] == (600, R.CLOSE_PROTOCOL, 1009)
    run_case(dev, c, "three tiles, first_bad 600")


def tiled_case(period, nseg, keyed):
    """(Case, the model's answer) of nseg segments: the Batch `period` repeated (PC.Tiled), a state
    word of 0 per segment, the keys of one period repeated when keyed. The model runs on one
    period; its per-segment answers are repeated and d_tx_off is the running sum of the repeated
    lengths, which is exact: every segment stands alone."""
    b = PC.Tiled(period, nseg)
    mf = b.max_frames
    pkeys = np.random.default_rng(7).integers(0, 1 << 32, period.nseg * (mf + 1), dtype=np.uint64).astype(np.uint32) if keyed else None
    tx, off, res, st = RC.Case(period, 0, None, None, pkeys, np.zeros(period.nseg, np.uint32)).expect()
    rest = int(off[nseg % period.nseg])
    exp = (tx * (nseg // period.nseg) + tx[:rest], np.concatenate([[0], np.cumsum(b.tile(np.diff(off)))]).astype(np.uint64),
           b.tile(res), b.tile(st))
    return RC.Case(b, 0, None, None, None if pkeys is None else b.tile(pkeys, mf + 1), np.zeros(nseg, np.uint32)), exp


@pytest.mark.parametrize("keyed", [False, True])
def test_more_than_1024_tiles(dev, keyed):
    """342 segments of 765 to 769 frames, 1026 tiles (tests/test_gpu_proto.py's batch): every thread
    of the one-block scan of the tile summaries takes two of them; a PONG's offset and what a
    segment sends need the tiles before. Pings stand before and after the CLOSE at frame 400."""
    period = PC.Batch(PC.long_period(), 769, gap=2)
    c, exp = tiled_case(period, 342, keyed)
    assert int(PC.list_starts(c.b)[-1]) + int(c.b.res["n_frames"][-1]) > 1024 * 256
    pings = [sum(1 for f in seg[:stop] if f[0] == 0x89) for seg, stop in zip(PC.long_period(), (769, 768, 400, 767, 768, 765))]
    assert pings[2] > 30 and sum(1 for f in PC.long_period()[2][401:] if f[0] == 0x89) > 30
    assert [tuple(int(v) for v in r)[:3] for r in exp[2][:6]] == [
        (pings[0], 0, 0), (pings[1], 0, 0), (pings[2], R.CLOSE_ECHO, 1000), (pings[3], 0, 0), (pings[4], R.CLOSE_ECHO, 1005),
        (pings[5], 0, 0)]
    run_case(dev, c, "1026 tiles keyed %d" % keyed, expect=exp)


def test_more_than_1024_plan_blocks(dev):
    """262 145 one-frame segments under max_frames 1: 1025 blocks of 256 segments, so every thread
    of the one-block scans of the frame counts and of the reply lengths takes two block sums"""
    c, exp = tiled_case(PC.Batch(PC.one_frame_period(), 1, gap=3), 262145, False)
    assert [tuple(int(v) for v in r) for r in exp[2][:7]] == [
        (0, 0, 0, 0), (0, 0, 0, 0), (0, R.CLOSE_ECHO, 1005, 4), (1, 0, 0, 4), (0, 0, 0, 0), (0, R.CLOSE_ECHO, 1000, 4), (1, 0, 0, 2)]
    assert [int(v) for v in exp[3][:7]] == [0, 0, 1, 0, 0, 1, 0]
    run_case(dev, c, "1025 plan blocks", expect=exp)


# ------------------------------------------------------------------ 4: packing

@pytest.mark.parametrize("nseg", [1, 3, 64, 65, 1000])
def test_packing_mixed_lengths(dev, nseg):
    """segments of mixed lengths sharing waves and blocks, empty ones and ones with no reply among
    them; a CLOSE in every fourth, a first_bad in every fifth, a fail status in every seventh"""
    rng = np.random.default_rng(nseg)
    lens = [int(rng.choice([0, 0, 1, 1, 2, 3, 5, 17, 63, 64, 65, 130, 300])) for _ in range(nseg)]
    segs, proto = [], []
    for s, n in enumerate(lens):
        fr = PC.quiet(n) if s % 3 else [PC.frame(PC.BIN, b"d")] * n
        if n and s % 4 == 0:
            fr[int(rng.integers(0, n))] = PC.close(1000 + s % 4)
        segs.append(fr)
        proto.append((int(rng.integers(0, n)), 1002) if n and s % 5 == 0 else (R.NONE, 0))
    b = PC.Batch(segs, 301, gap=2)
    fail = np.zeros(nseg, np.uint32)
    fail[::7] = 1007
    state = np.zeros(nseg, np.uint32)
    state[::11] = R.ST_CLOSE_SENT
    c = RC.Case(b, 0, proto, fail, None, state)
    exp = c.expect()
    assert (np.diff(exp[1].astype(np.int64)) >= 0).all() and (nseg < 64 or (exp[2]["tx_len"] == 0).sum() > 5)
    run_case(dev, c, "packing %d" % nseg)
    run_case(dev, c, "packing %d, wire masked, most recent" % nseg, flags=WM | LAST)


# ------------------------------------------------------------------ 5: precedence and liveness

def test_precedence_and_liveness(dev):
    f, p = PC.frame, PC.PING
    conn = [f(p, b"1"), f(PC.TEXT, b"t"), f(p, b"2"), PC.close(1000), f(p, b"3")]
    big = PC.close(4000, b"r" * 123)
    segs = [conn, conn, conn, conn, conn, [f(p, b"1"), f(p, b"2")], [f(p, b"1"), PC.close()], [PC.close(reason=b"x")], [big],
            conn]
    proto = [(1, 1002), (3, 1002), (4, 1009), (R.NONE, 0), (R.NONE, 0), (R.NONE, 0), (R.NONE, 0), (R.NONE, 0), (R.NONE, 0),
             (2, 1009)]
    fail = np.array([0, 0, 0, 1001, 0, 1007, 0, 0, 0, 1001], np.uint32)
    b = PC.Batch(segs, 6, gap=1)
    c = RC.Case(b, 0, proto, fail, None, np.zeros(len(segs), np.uint32))
    exp = c.expect()
    assert [tuple(int(v) for v in r)[:3] for r in exp[2]] == [
        (1, 2, 1002), (2, 2, 1002), (2, 1, 1000), (2, 3, 1001), (2, 1, 1000), (2, 3, 1007), (1, 1, 0), (0, 1, 0), (0, 1, 4000),
        (1, 2, 1009)]
    run_case(dev, c, "precedence")
    c2 = RC.Case(b, LAST, proto, fail, None, np.zeros(len(segs), np.uint32))
    assert [int(v) for v in c2.expect()[2]["n_pong"]] == [1, 1, 1, 1, 1, 1, 1, 0, 0, 1]
    run_case(dev, c2, "precedence, most recent ping")
    run_case(dev, c2, "precedence, wire masked", flags=WM | LAST)


# ------------------------------------------------------------------ 6: capacity

def test_capacity(dev):
    rows = RC.table_groups()[0]
    c = RC.table_case(rows)
    exp = RC.table_expect(rows)
    off = [int(v) for v in exp[1]]
    total = off[-1]
    inside_body = next(o + 40 for o, n in zip(off, off[1:]) if n - o > 100)
    edge = next(o for o in off if o > 130)
    for cap in (0, 1, off[1] + 1, inside_body, edge, total - 1, total):
        run_case(dev, c, "capacity %d" % cap, cap=cap, expect=exp)


# ------------------------------------------------------------------ 7: carry

def test_carry_every_cut(dev):
    """the script cut into two and into three batches at every frame boundary: the reply bytes
    side by side equal the one-batch reply and the last state matches; with CLOSE_SENT on entry
    nothing is written; with no state every batch stands alone"""
    frames = short_script()
    n = len(frames)
    whole = RC.Case(PC.Batch([frames], n), 0, None, None, None, np.zeros(1, np.uint32))
    wtx, _woff, wres, wst = whole.expect()
    assert tuple(wres[0])[:3] == (3, R.CLOSE_ECHO, 1001) and wst[0] == R.ST_CLOSE_SENT
    run_case(dev, whole, "whole")
    for a, c_ in [(a, n) for a in range(n + 1)] + [(a, c_) for a in range(n + 1) for c_ in range(a, n + 1)]:
        state, got = np.zeros(1, np.uint32), b""
        for part in (frames[:a], frames[a:c_], frames[c_:]):
            c = RC.Case(PC.Batch([part], n), 0, None, None, None, state)
            exp = c.expect()
            state = run_case(dev, c, "cut %d,%d" % (a, c_))
            got += exp[0]
        assert got == wtx and state[0] == wst[0], (a, c_)
    tail = RC.Case(PC.Batch([frames[5:]], n), 0, None, None, None, np.ones(1, np.uint32))
    assert tail.expect()[0] == b"" and tuple(tail.expect()[2][0]) == (0, 0, 0, 0)
    run_case(dev, tail, "close sent on entry")
    alone = tail.expect(state=None)
    assert alone[0] == b"\x8a\x04late\x88\x02\x03\xe8"
    run_case(dev, tail, "no state", state=None)


# ------------------------------------------------------------------ 8: client role

def test_client_role_replies_decode_to_plain_bodies(dev):
    """with keys every frame carries its slot's key (the model's bytes); the batch decode over
    d_tx, one segment per connection, then yields the bodies of the server-role reply"""
    for i, c in enumerate(x for x in RC.random_cases() if x.keys is not None):
        b = c.b
        exp = c.expect()
        run_case(dev, c, "client %d" % i)
        etx, eoff = exp[0], exp[1]
        plain = RC.Case(b, c.flags, None, c.fail, None, c.state)
        plain.proto = c.proto
        ptx, poff, _, _ = plain.expect()
        tx = up(dev, np.frombuffer(etx + b"\0" * PC.PAD, np.uint8).copy())
        mf = b.max_frames + 1
        desc = torch.zeros(32 * b.nseg * mf, dtype=torch.uint8, device=dev)
        res = torch.zeros(16 * b.nseg, dtype=torch.uint8, device=dev)
        W.batch_decode_device(tx, i64(dev, eoff[:-1]), i64(dev, np.diff(eoff.astype(np.int64))), mf, desc, res)
        torch.cuda.synchronize()
        gd, gr, gt = desc.cpu().numpy().view(W.DESC_DTYPE), res.cpu().numpy().view(W.SEGRES_DTYPE), tx.cpu().numpy()
        for s in range(b.nseg):
            bodies = b"".join(bytes(gt[int(d["data_off"]):int(d["data_off"]) + int(d["datalen"])])
                              for d in gd[s * mf:s * mf + int(gr[s]["n_frames"])] if int(d["datalen"]))
            server = ptx[int(poff[s]):int(poff[s + 1])]
            want, pos = b"", 0
            while pos < len(server):
                want += server[pos + 2:pos + 2 + server[pos + 1]]
                pos += 2 + server[pos + 1]
            assert int(gr[s]["consumed"]) == int(eoff[s + 1] - eoff[s]) and bodies == want, (i, s)


def test_seeded_random(dev):
    """the builders and seed whose coverage tests/test_reply_host.py asserts"""
    for i, c in enumerate(RC.random_cases()):
        run_case(dev, c, "random %d" % i)
        run_case(dev, c, "random %d, no state" % i, state=None)


# ------------------------------------------------------------------ 9: chain and capture

def test_capture_decode_check_reply(dev):
    """decode, check, reply captured as one chain after a warm call and replayed on two wires of
    one shape; the workspace does not grow between replays"""
    lib = _lib.load_reply_lib()
    shapes = [[1, 2, 0, 3, 1], [2, 1], [0, 1, 3, 2] * 80]

    def wires(kind):
        segs = []
        for s, sizes in enumerate(shapes):
            fr = []
            for i, n in enumerate(sizes):
                op = PC.PING if (i + kind) % 3 == 0 else PC.BIN
                fr.append(PC.frame(op, bytes([65 + kind + i % 7]) * n, rsv=0x40 if kind == 2 and i == 300 else 0))
            if kind == 2 and s == 1:
                fr[1] = PC.frame(PC.CLOSE, b"\x03")              # same length as the frame it replaces: one body byte
            segs.append(fr)
        return PC.Batch(segs, 330, gap=4)

    b0 = wires(1)
    t = device_batch(dev, b0)
    n, mf = b0.nseg, 330
    pres = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    rres = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    pst = torch.zeros(n, dtype=torch.int64, device=dev)
    rst = torch.zeros(n, dtype=torch.int32, device=dev)
    tx = torch.full((131 * n * mf // 8,), FILL, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)

    def call():
        s = torch.cuda.current_stream().cuda_stream
        p = lambda x: x.data_ptr()                               # noqa: E731
        rc = lib.websocketframeBatchDecodeDevice(p(t["d"]), t["d"].numel() - PC.PAD, p(t["so"]), p(t["sl"]), n, mf, None,
                                                 p(t["desc"]), p(t["res"]), s)
        rc |= lib.websocketframeBatchCheckProtocolDevice(p(t["d"]), p(t["so"]), p(t["desc"]), p(t["res"]), n, mf,
                                                         P.EXPECT_MASKED, 0, 0, p(pst), None, p(pres), s)
        rc |= lib.websocketframeBatchControlRepliesDevice(p(t["d"]), p(t["so"]), p(t["desc"]), p(t["res"]), n, mf, 0, p(pres), None,
                                                          None, p(rst), p(tx), tx.numel(), p(off), p(rres), s)
        assert rc == 0, lib.websocketframeGpuLastError()

    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    stat = C.c_ulonglong(0)
    held = []
    for kind in (1, 2):
        b = wires(kind)
        assert b.seg_off == b0.seg_off and len(b.raw) == len(b0.raw)
        t["d"].copy_(up(dev, b.raw))
        pst.zero_()
        rst.zero_()
        tx.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        _codes, eproto, _w = b.expect(P.EXPECT_MASKED, 0, 0, np.zeros(n, np.uint64))
        c = RC.Case(b, 0, None, None, None, np.zeros(n, np.uint32))
        c.proto = eproto
        etx, eoff, eres, est = c.expect()
        assert np.array_equal(pres.cpu().numpy().view(P.RES_DTYPE), eproto), kind
        assert np.array_equal(off.cpu().numpy().view(np.uint64), eoff), kind
        assert np.array_equal(rres.cpu().numpy().view(R.RES_DTYPE), eres), kind
        assert np.array_equal(rst.cpu().numpy().view(np.uint32), est), kind
        got = tx.cpu().numpy()
        assert bytes(got[:len(etx)]) == etx and (got[len(etx):] == FILL).all(), kind
        assert (eres["close_kind"] == R.CLOSE_PROTOCOL).sum() == (2 if kind == 2 else 0) and int(eres["n_pong"].sum()) >= 90
        assert lib.websocketframeGpuGetStat(b"workspace_bytes", C.byref(stat)) == 0
        held.append(stat.value)
    assert held[0] == held[1] > 0
    del g


# ------------------------------------------------------------------ 10: argument errors

def test_argument_errors(dev):
    lib = _lib.load_reply_lib()
    c = RC.table_case(RC.table_groups()[0])
    b = c.b
    d, so, desc, res = up(dev, b.dec), i64(dev, b.seg_off), up(dev, b.desc), up(dev, b.res)
    tx = torch.full((4096,), FILL, dtype=torch.uint8, device=dev)
    off = torch.full((b.nseg + 1,), 0x6E6E6E6E, dtype=torch.int64, device=dev)
    rres = torch.full((16 * b.nseg,), FILL, dtype=torch.uint8, device=dev)
    st = torch.full((b.nseg,), 0x6E6E6E6E, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    ptr = dict(d=d.data_ptr(), so=so.data_ptr(), desc=desc.data_ptr(), res=res.data_ptr(), tx=tx.data_ptr(), off=off.data_ptr(),
               rres=rres.data_ptr())

    def call(nseg=b.nseg, mf=b.max_frames, flags=0, cap=4096, **kw):
        a = dict(ptr, **kw)
        return lib.websocketframeBatchControlRepliesDevice(a["d"], a["so"], a["desc"], a["res"], nseg, mf, flags, None, None, None,
                                                           st.data_ptr(), a["tx"], cap, a["off"], a["rres"], s)
    for kw, word in ((dict(flags=1), b"flag"), (dict(flags=2), b"flag"), (dict(flags=0x80000000), b"flag"),
                     (dict(mf=0), b"max_frames"), (dict(d=None), b"NULL"), (dict(so=None), b"NULL"), (dict(desc=None), b"NULL"),
                     (dict(res=None), b"NULL"), (dict(off=None), b"NULL"), (dict(rres=None), b"NULL"), (dict(tx=None), b"NULL"),
                     (dict(nseg=0, flags=16), b"flag"), (dict(nseg=0, off=None), b"NULL"), (dict(nseg=1 << 20, mf=1 << 11), b"2^30")):
        assert call(**kw) < 0, kw
        assert word in lib.websocketframeGpuLastError(), kw
    torch.cuda.synchronize()
    assert (tx == FILL).all() and (off == 0x6E6E6E6E).all() and (rres == FILL).all() and (st == 0x6E6E6E6E).all()
    assert call(nseg=0, d=None, so=None, desc=None, res=None, rres=None, tx=None, cap=0) == 0      # d_tx_off[0] = 0 only
    torch.cuda.synchronize()
    assert int(off[0]) == 0 and (off[1:] == 0x6E6E6E6E).all() and (tx == FILL).all() and (rres == FILL).all()
    assert (st == 0x6E6E6E6E).all()


# ------------------------------------------------------------------ 11: offsets past 4 GiB

def test_ping_body_and_close_status_straddle_4gib(dev):
    """the wire placed so that a masked ping's body, then a masked CLOSE's two status bytes,
    straddle arena offset 2^32: descriptors rebased, the arena's window and its low aliases
    unchanged"""
    H.need_memory(torch, pytest)
    segs = [[PC.frame(PC.PING, b"0123456789abcdefghij")], [PC.frame(PC.PING, b"p"), PC.close(0x3412, b"why")]]
    b = PC.Batch(segs, 3, gap=5)
    c = RC.Case(b, WM, None, None, None, np.zeros(2, np.uint32))
    exp = c.expect()
    assert exp[0] == b"\x8a\x140123456789abcdefghij\x8a\x01p\x88\x02\x34\x12"
    arena = H.Arena(dev)
    img = b.raw[:-PC.PAD]
    for what, at in (("ping body", int(b.desc[0]["data_off"]) + 7), ("close status", int(b.desc[3 + 1]["data_off"]) + 1)):
        high = H.place(H.B32, at)
        placed = arena.put(high, img)
        lo, hi = H.window(high, len(img))
        check_call(dev, arena.view(high, len(img)), i64(dev, [o + high for o in b.seg_off]), up(dev, H.rebase(b.desc, high)),
                   up(dev, b.res), b.nseg, 3, WM, None, None, None, c.state, exp, "2^32 " + what, window=(lo, hi))
        arena.check(placed, img, "2^32 " + what)
