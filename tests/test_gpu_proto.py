"""websocketframeBatchCheckProtocolDevice (libwsframe_amd_proto.so) on the GPU against the
sequential oracle (proto_oracle.py) and the hand-written directed table (proto_cases.py). Every
call compares every output of every segment: d_frame_code slot for slot (a 0xEE fill must be
intact wherever nothing is to be written), d_proto_res, d_proto_state, and the bytes of d_buf,
d_desc and d_res, which must come back unchanged."""
import ctypes as C

import numpy as np
import pytest

import high_arena as H
import proto_cases as PC
import proto_oracle as P
from util_amd import _lib
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = P.FILL
EM, EU, WM = P.EXPECT_MASKED, P.EXPECT_UNMASKED, P.WIRE_MASKED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.load_proto_lib()                                    # a missing library fails here, it never skips
    return torch.device("cuda:0")


def up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)


def i64(dev, a):
    return torch.from_numpy(np.asarray(a, np.uint64).astype(np.int64)).to(dev)


def check_call(dev, d_buf, d_so, d_desc, d_res, nseg, mf, flags, rsv, limit, state, expect, tag, codes=True, window=None):
    """one call on device tensors; state: numpy u64 in (None: NULL); expect: (codes, res, words) of
    the oracle. Returns the state words out."""
    ecodes, eres, ewords = expect
    code_t = torch.full((max(1, nseg * mf),), FILL, dtype=torch.uint8, device=dev) if codes else None
    res_t = torch.full((max(1, nseg) * 16,), FILL, dtype=torch.uint8, device=dev)
    st_t = None if state is None else i64(dev, state)
    seen = d_buf if window is None else d_buf[window[0]:window[1]]
    before = [t.clone() for t in (seen, d_desc, d_res)]
    W.batch_check_protocol_device(d_buf, d_so, d_desc, d_res, mf, res_t, flags, rsv, limit, st_t, code_t)
    torch.cuda.synchronize()
    for t, b, name in zip((seen, d_desc, d_res), before, ("d_buf", "d_desc", "d_res")):
        assert torch.equal(t, b), "%s: %s modified" % (tag, name)
    gres = res_t.cpu().numpy().view(P.RES_DTYPE)[:nseg]
    bad = np.nonzero(gres != eres)[0]
    assert not len(bad), "%s: segment %d result %s, oracle %s" % (tag, bad[0], gres[bad[0]], eres[bad[0]])
    if codes:
        g = code_t.cpu().numpy()[:nseg * mf]
        bad = np.nonzero(g != ecodes)[0]
        assert not len(bad), "%s: segment %d frame %d code %#x, oracle %#x (%d slots differ)" % (
            tag, bad[0] // mf, bad[0] % mf, g[bad[0]], ecodes[bad[0]], len(bad))
    if state is None:
        return None
    gw = st_t.cpu().numpy().view(np.uint64)
    bad = np.nonzero(gw != ewords)[0]
    assert not len(bad), "%s: segment %d state %x -> %x, oracle %x" % (tag, bad[0], state[bad[0]], gw[bad[0]], ewords[bad[0]])
    return gw


def run_batch(dev, b, flags=0, rsv=0, limit=0, state=None, tag="", codes=True):
    """a Batch's oracle descriptors on the device, the wire as the flags say (still masked under
    WIRE_MASKED, else as the in-place decode leaves it)"""
    wire = b.raw if flags & WM else b.dec
    return check_call(dev, up(dev, wire), i64(dev, b.seg_off), up(dev, b.desc), up(dev, b.res), b.nseg, b.max_frames,
                      flags, rsv, limit, state, b.expect(flags, rsv, limit, state), tag, codes)


# ------------------------------------------------------------------ 1 + 2: the table, behind every feeder

def device_batch(dev, b):
    """the Batch's raw wire and output buffers on the device"""
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


def table_groups():
    groups = {}
    for row in PC.directed_table():
        groups.setdefault((row[2], row[3]), []).append(row)
    return groups


@pytest.mark.parametrize("feeder", ["decode", "reasm", "ex", "ctl"])
def test_directed_table(dev, feeder):
    """Autobahn 2, 3, 4, 5 and 7, one connection per segment, against the codes written by hand in
    the table; descriptors from the in-place decode and from the three reassembly calls (the
    wire still masked: WIRE_MASKED)"""
    for (flags, rsv), rows in table_groups().items():
        b = PC.Batch([r[1] for r in rows], max(len(r[1]) for r in rows) + 1, gap=3)
        ecodes = np.full(b.nseg * b.max_frames, FILL, np.uint8)
        eres = np.zeros(b.nseg, P.RES_DTYPE)
        for s, (_name, frames, _f, _r, codes, first_bad, code, status, close_frame) in enumerate(rows):
            ecodes[s * b.max_frames:s * b.max_frames + len(codes)] = codes
            eres[s] = (first_bad, code, status, close_frame)
        d_buf, d_desc, d_res, wm = feed(dev, b, feeder)
        check_call(dev, d_buf, i64(dev, b.seg_off), d_desc, d_res, b.nseg, b.max_frames, flags | wm, rsv, 0, None,
                   (ecodes, eres, None), "table %s flags %d rsv %#x" % (feeder, flags, rsv))


def close_script():
    """masked CLOSE frames whose status code is valid only after unmasking (1000 reads 0x3412 on
    the wire) and only before it (0x3412 reads 1000 on the wire), between data frames"""
    return [[PC.frame(PC.TEXT, b"ab"), PC.close(1000), PC.frame(PC.PING)],
            [PC.frame(PC.BIN, b"c", fin=0), PC.frame(PC.CONT, b"d"), PC.close(0x3412)],
            [PC.close(1001, b"x", masked=False)],
            [PC.frame(PC.PING, b"p"), PC.close(0x3412, masked=False)]]


@pytest.mark.parametrize("feeder", ["decode", "reasm", "ex", "ctl"])
def test_feeders_close_code_masking(dev, feeder):
    b = PC.Batch(close_script(), 4, gap=5)
    d_buf, d_desc, d_res, wm = feed(dev, b, feeder)
    state = np.zeros(b.nseg, np.uint64)
    exp = b.expect(wm, 0, 0, state)
    assert [int(c) for c in exp[1]["code"]] == [0, 7, 0, 7]
    check_call(dev, d_buf, i64(dev, b.seg_off), d_desc, d_res, b.nseg, 4, wm, 0, 0, state, exp, "close " + feeder)
    # the wrong flag for the feeder reads the other bytes: the verdicts of the masked frames swap
    wrong = P.check(b.raw if wm else b.dec, b.seg_off, b.desc, b.res, 4, wm ^ WM, 0, 0, state)
    assert [int(c) for c in wrong[1]["code"]] == [7, 0, 0, 7]


def test_feeder_stream_decode(dev):
    """one raw stream: descriptors from websocketframeStreamDecodeDevice, one segment at offset 0"""
    frames = PC.quiet(300) + [PC.frame(PC.CONT, b"z")] + PC.quiet(299, tail_open=True) + [PC.close(1005), PC.frame(PC.PING)]
    b = PC.Batch([frames], len(frames) + 3)
    d = up(dev, b.raw)
    desc = torch.zeros(32 * b.max_frames, dtype=torch.uint8, device=dev)
    res = torch.zeros(16, dtype=torch.uint8, device=dev)
    W.stream_decode_device(d, b.seg_len[0], b.max_frames, desc, res)
    state = np.zeros(1, np.uint64)
    exp = b.expect(EM, 0, 0, state)
    assert tuple(exp[1][0]) == (300, 8, 1002, 600) and exp[2][0] == P.ST_OPEN | P.ST_CLOSED | 1
    check_call(dev, d, i64(dev, [0]), desc, res, 1, b.max_frames, EM, 0, 0, state, exp, "stream")


# ------------------------------------------------------------------ 3: tile and packing edges

LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1030]
EDGES = [254, 255, 256, 257, 258, 510, 511, 512, 513, 514]


def test_segment_lengths(dev):
    """segments of every length around the wave and the tile, valid and left open, in one batch"""
    b = PC.Batch([PC.quiet(n, tail_open=bool(i & 1)) for i, n in enumerate(LENGTHS)], 1030)
    state = np.zeros(b.nseg, np.uint64)
    gw = run_batch(dev, b, EM, 0, 0, state, "lengths")
    assert [bool(w & P.ST_OPEN) for w in gw] == [bool(i & 1) and n > 0 for i, n in enumerate(LENGTHS)]
    run_batch(dev, b, EM, 0, 0, None, "lengths, no state", codes=False)


def list_pos(b, s, k):
    """where frame k of segment s stands in the list of the batch's frames that the kernels cut
    into tiles of 256"""
    return int(PC.list_starts(b)[s]) + k


@pytest.mark.parametrize("shift", [0, 100])
def test_single_error_at_every_tile_edge(dev, shift):
    """one error of each kind at the list positions 254..258 and 510..514 past a tile's start of an
    otherwise valid connection, each in a segment of its own, the kinds turning. Every segment is
    768 frames long and the batch starts with `shift` filler frames, so a segment's frame k stands
    at list position k + shift mod 256: with shift 0 the tile edges are the segment's k = 256 and
    512, with shift 100 its k = 156 and 412."""
    segs, at = [PC.quiet(shift)], []
    for i, e in enumerate(EDGES):
        for j in range(3):
            kind = PC.PLAIN[(3 * i + j) % 8] if j < 2 else 6 + i % 2
            k = e - shift
            head = PC.quiet(k, tail_open=kind in (9, 10))
            segs.append(head + [PC.error_frame(kind, kind in (9, 10), 2, 1)] + PC.quiet(768 - k - 1))
            at.append(k)
    b = PC.Batch(segs, 768, gap=1)
    exp = b.expect(EM, 0, 2, None)
    assert [int(f) for f in exp[1]["first_bad"][1:]] == at and set(int(c) for c in exp[1]["code"][1:]) == set(range(1, 11))
    assert sorted({list_pos(b, s + 1, k) % 256 for s, k in enumerate(at)}) == [0, 1, 2, 254, 255]
    run_batch(dev, b, EM, 0, 2, None, "edges")
    run_batch(dev, b, EM, 0, 2, np.zeros(b.nseg, np.uint64), "edges with state")


@pytest.mark.parametrize("shift", [0, 100])
@pytest.mark.parametrize("edge", [256, 512])
def test_open_message_and_limit_across_a_tile_edge(dev, edge, shift):
    """one message of one-byte fragments from frame 0 on: `bytes` before frame k is k, so a limit L
    stops frame k = L; L puts that frame exactly at, one before and one after the tile edge (list
    position `edge`: the segments are 768, 256 and 769 frames long after `shift` filler frames);
    a ping on the edge does not count"""
    frames = [PC.frame(PC.TEXT, b"a", fin=0)] + [PC.frame(PC.CONT, b"b", fin=0) for _ in range(767)]
    cut = edge - shift
    b = PC.Batch([PC.quiet(shift), frames, PC.quiet(256), frames[:cut] + [PC.frame(PC.PING)] + frames[cut:]], 769)
    assert [list_pos(b, s, cut) % 256 for s in (1, 3)] == [0, 0]
    for limit in (cut - 1, cut, cut + 1):
        state = np.zeros(4, np.uint64)
        exp = b.expect(0, 0, limit, state)
        assert [int(f) for f in exp[1]["first_bad"]] == [P.NONE, limit, P.NONE, limit + (limit >= cut)]
        assert [int(c) for c in exp[1]["close_status"]] == [0, 1009, 0, 1009] and exp[2][1] == P.ST_OPEN | 768
        run_batch(dev, b, 0, 0, limit, state, "limit %d" % limit)
    # the same through a carried count: the message is 7 bytes long already
    state = np.array([0, P.ST_OPEN | 7, 0, P.ST_OPEN | 7], np.uint64)
    cont = [PC.frame(PC.CONT, b"b", fin=0)] + frames[1:]
    b = PC.Batch([PC.quiet(shift), cont, PC.quiet(256), cont], 769)
    exp = b.expect(0, 0, cut + 7, state)
    assert [int(f) for f in exp[1]["first_bad"]] == [P.NONE, cut, P.NONE, cut]
    run_batch(dev, b, 0, 0, cut + 7, state, "carried limit")


@pytest.mark.parametrize("shift", [0, 100])
def test_first_close_at_a_tile_edge(dev, shift):
    """the first CLOSE on a tile's last frame, on the next tile's first and second (segments of 512
    frames after `shift` filler frames)"""
    ks = [e - shift for e in (255, 256, 257)]
    segs = [PC.quiet(shift)] + [PC.quiet(k) + [PC.close(1000)] + PC.quiet(510 - k) + [PC.close(1005)] for k in ks]
    b = PC.Batch(segs, 512)
    assert [list_pos(b, s + 1, k) % 256 for s, k in enumerate(ks)] == [255, 0, 1]
    state = np.zeros(4, np.uint64)
    exp = b.expect(EM, 0, 0, state)
    assert [int(c) for c in exp[1]["close_frame"][1:]] == ks and (exp[1]["first_bad"] == P.NONE).all()
    assert (exp[2][1:] == P.ST_CLOSED).all()
    run_batch(dev, b, EM, 0, 0, state, "close at the edge")


@pytest.mark.parametrize("nseg", [1, 3, 64, 65, 1000])
def test_packing_mixed_lengths(dev, nseg):
    """segments of mixed lengths, empty ones among them, sharing waves and blocks; an error in
    every third"""
    rng = np.random.default_rng(nseg)
    lens = [int(rng.choice([0, 0, 1, 1, 2, 3, 5, 17, 63, 64, 65, 130, 300])) for _ in range(nseg)]
    segs = []
    for s, n in enumerate(lens):
        fr = PC.quiet(n, tail_open=s % 5 == 0)
        if n and s % 3 == 0:
            fr[int(rng.integers(0, n))] = PC.error_frame(int(rng.choice([1, 2, 4, 5])), False, 0)
        segs.append(fr)
    b = PC.Batch(segs, 301, gap=2)
    state = np.zeros(nseg, np.uint64)
    state[::7] = P.ST_OPEN | 3
    run_batch(dev, b, EM, 0, 0, state, "packing %d" % nseg)


def test_max_frames_one(dev):
    segs = [[PC.frame(PC.TEXT, b"a", fin=0), PC.frame(PC.CONT, b"b")], [PC.frame(PC.CONT, b"c")], [], [PC.close(1005)]]
    b = PC.Batch(segs, 1)
    assert [int(s) for s in b.res["status"]] == [W.SEG_MAX_FRAMES, 0, 0, 0]
    state = np.zeros(4, np.uint64)
    exp = b.expect(0, 0, 0, state)
    assert [int(c) for c in exp[1]["code"]] == [0, 8, 0, 7] and exp[2][0] == P.ST_OPEN | 1
    run_batch(dev, b, 0, 0, 0, state, "max_frames 1")


def test_more_than_1024_plan_blocks(dev):
    """262 145 one-frame segments under max_frames 1: 1025 plan blocks of 256 segments (and 1025
    tiles), so every thread of the one-block scan of the block sums takes two of them. The batch
    is a period of seven segments repeated (PC.Tiled), every segment compared."""
    b = PC.Tiled(PC.Batch(PC.one_frame_period(), 1, gap=3), 262145)
    state = np.zeros(b.nseg, np.uint64)
    exp = b.expect(EM, 0, 0, state)
    assert [int(c) for c in exp[1]["code"][:7]] == [0, 8, 7, 0, 0, 0, 0] and exp[2][0] == P.ST_OPEN | 1
    assert [int(c) for c in exp[1]["close_frame"][:7]] == [P.NONE, P.NONE, 0, P.NONE, P.NONE, 0, P.NONE]
    run_batch(dev, b, EM, 0, 0, state, "1025 plan blocks")


def test_more_than_1024_tiles(dev):
    """342 segments of 765 to 769 frames, 1026 tiles: every thread of the one-block scan of the tile
    summaries takes two of them. A period of six segments repeated (PC.Tiled), each three tiles
    long and more and 255 list positions further on in every period, so the tile edges fall
    everywhere; the error behind 700 bytes of an open message, the open message a TEXT frame
    interrupts, the frames after a CLOSE and the state words all need the tiles before."""
    b = PC.Tiled(PC.Batch(PC.long_period(), 769, gap=2), 342)
    assert int(PC.list_starts(b)[-1]) + int(b.res["n_frames"][-1]) > 1024 * 256
    state = np.zeros(b.nseg, np.uint64)
    exp = b.expect(EM, 0, 700, state)
    assert [int(f) for f in exp[1]["first_bad"][:6]] == [700, 501, P.NONE, P.NONE, 768, P.NONE]
    assert [int(c) for c in exp[1]["code"][:6]] == [10, 9, 0, 0, 7, 0] and int(exp[1]["close_frame"][2]) == 400
    assert (exp[0][2 * 769 + 401:3 * 769] == P.AFTER_CLOSE).all()
    assert [int(w) for w in exp[2][:6]] == [P.ST_OPEN | 769, 0, P.ST_CLOSED, P.ST_OPEN | 2, P.ST_CLOSED, 0]
    run_batch(dev, b, EM, 0, 700, state, "1026 tiles")


# ------------------------------------------------------------------ 4: frames that are not consumed

def test_not_consumed(dev):
    """segments stopped by MAX_FRAMES, by an incomplete tail, by ERR_DECODE (the negative ret of a
    frame of >= 2 GiB: its descriptor, hand-built) and by the cache limit (descriptors from
    websocketframeBatchReassembleDeviceEx with a small limit)"""
    tail = PC.frame(PC.TEXT, b"abc")[:-2]
    segs = [PC.quiet(6), [PC.frame(PC.TEXT, b"a", fin=0), PC.frame(PC.CONT, b"b"), tail],
            [PC.frame(PC.PING), PC.frame(PC.CONT, b"x"), PC.frame(PC.BIN, b"y")], PC.quiet(2)]
    b = PC.Batch(segs, 4)
    b.unconsume_last(2, -1)
    assert [int(s) for s in b.res["status"]] == [W.SEG_MAX_FRAMES, 0, W.SEG_ERR_DECODE, 0]
    state = np.zeros(4, np.uint64)
    exp = b.expect(EM, 0, 0, state)
    assert exp[0][2 * 4 + 2] == P.NOT_CONSUMED and tuple(exp[1][2]) == (1, 8, 1002, P.NONE)
    run_batch(dev, b, EM, 0, 0, state, "not consumed")
    # the cache limit: the third fragment would take the cached bytes past 5
    segs = [[PC.frame(PC.TEXT, b"abc", fin=0), PC.frame(PC.CONT, b"de", fin=0), PC.frame(PC.CONT, b"f", fin=0),
             PC.close(1005)], PC.quiet(3)]
    b = PC.Batch(segs, 5)
    t = device_batch(dev, b)
    W.batch_reassemble_device(t["d"], t["so"], t["sl"], 5, t["desc"], t["res"], t["out"], t["msg"], t["nmsg"], readcache_max=5)
    torch.cuda.synchronize()
    gres = t["res"].cpu().numpy().view(W.SEGRES_DTYPE)
    assert int(gres[0]["status"]) == W.SEG_ERR_CACHE_OVERFLOW and int(gres[0]["n_frames"]) == 3
    b.res = gres.copy()                                       # the oracle judges what the call reported
    exp = b.expect(WM, 0, 0, state[:2])
    assert list(exp[0][:5]) == [0, 0, P.NOT_CONSUMED, FILL, FILL] and exp[2][0] == P.ST_OPEN | 5
    check_call(dev, t["d"], t["so"], t["desc"], t["res"], 2, 5, WM, 0, 0, state[:2], exp, "cache overflow")


# ------------------------------------------------------------------ 5: carry across batches

def test_carry_every_cut(dev):
    """the nine-frame script cut into two and into three batches at every frame boundary: the
    codes side by side and the last state equal the one-batch run; with no state every batch
    stands alone; the limit is reached through the carried bytes"""
    frames = PC.carry_script()
    n = len(frames)
    whole = PC.Batch([frames], n)
    wc, wr, ww = whole.expect(EM, 0, 6, np.zeros(1, np.uint64))
    assert list(wc[:n]) == [0, 0, 0, 0, 10, 0, 0, 0, P.AFTER_CLOSE] and ww[0] == P.ST_OPEN | P.ST_CLOSED | 1
    run_batch(dev, whole, EM, 0, 6, np.zeros(1, np.uint64), "whole")
    cuts = [(a, n) for a in range(n + 1)] + [(a, c) for a in range(n + 1) for c in range(a, n + 1)]
    for a, c in cuts:
        state = np.zeros(1, np.uint64)
        got = []
        for part in (frames[:a], frames[a:c], frames[c:]):
            b = PC.Batch([part], n)
            exp = b.expect(EM, 0, 6, state)
            state = run_batch(dev, b, EM, 0, 6, state, "cut %d,%d" % (a, c))
            got += list(exp[0][:len(part)])
            run_batch(dev, b, EM, 0, 6, None, "cut %d,%d alone" % (a, c))
        assert got == list(wc[:n]) and state[0] == ww[0], (a, c)
    alone = PC.Batch([frames[3:]], n).expect(EM, 0, 6, None)
    assert alone[0][0] == P.ERR_CONT_UNEXPECTED and alone[0][1] == 0     # no carried bytes, no carried message


# ------------------------------------------------------------------ 6: seeded random

def test_seeded_random(dev):
    """the builders and seed whose coverage tests/test_proto_host.py asserts"""
    for i, (b, flags, rsv, limit, state) in enumerate(PC.random_cases()):
        run_batch(dev, b, flags, rsv, limit, state, "random %d" % i)
        run_batch(dev, b, flags, rsv, limit, None, "random %d, no state, no codes" % i, codes=False)


# ------------------------------------------------------------------ 7: argument errors

def test_argument_errors(dev):
    lib = _lib.load_proto_lib()
    b = PC.Batch(close_script(), 4)
    d, so, desc, res = up(dev, b.dec), i64(dev, b.seg_off), up(dev, b.desc), up(dev, b.res)
    code = torch.full((16,), FILL, dtype=torch.uint8, device=dev)
    pres = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    st = torch.full((4,), 0x6E6E6E6E, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def call(nseg, flags, rsv, mf=4):
        return lib.websocketframeBatchCheckProtocolDevice(d.data_ptr(), so.data_ptr(), desc.data_ptr(), res.data_ptr(), nseg,
                                                          mf, flags, rsv, 0, st.data_ptr(), code.data_ptr(), pres.data_ptr(), s)
    for flags, rsv, mf, word in ((8, 0, 4, b"flag"), (EM | EU, 0, 4, b"EXPECT"), (0x80000000, 0, 4, b"flag"),
                                 (0, 0x80, 4, b"rsv_allowed"), (0, 0x71, 4, b"rsv_allowed"), (0, 0, 0, b"invalid")):
        assert call(4, flags, rsv, mf) < 0
        assert word in lib.websocketframeGpuLastError()
    assert call(0, 8, 0) < 0                                   # the flags are judged before nseg
    assert call(0, 0, 0) == 0
    torch.cuda.synchronize()
    assert (code == FILL).all() and (pres == FILL).all() and (st == 0x6E6E6E6E).all()


# ------------------------------------------------------------------ 8: graph capture

def test_capture_decode_then_check(dev):
    """decode then check captured as one linear chain after a warm call, replayed on two wires of
    the same shape; the workspace does not grow between replays"""
    lib = _lib.load_proto_lib()
    shapes = [[1, 2, 0, 3, 1], [2, 1], [0, 1, 3, 2] * 80]

    def wires(kind):
        segs = []
        for s, sizes in enumerate(shapes):
            fr = []
            for i, n in enumerate(sizes):
                op = (PC.TEXT if kind == 1 else PC.BIN) if i % 2 == 0 else PC.CONT
                fin = i % 2 if kind == 1 else (i + s) % 2
                fr.append(PC.frame(op, b"w" * n, fin=fin, rsv=0x40 if kind == 2 and i == 7 else 0))
            segs.append(fr)
        return PC.Batch(segs, 330, gap=4)

    b0 = wires(1)
    t = device_batch(dev, b0)
    n = b0.nseg
    code = torch.full((n * 330,), FILL, dtype=torch.uint8, device=dev)
    pres = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    st = torch.zeros(n, dtype=torch.int64, device=dev)

    def call():
        W.batch_decode_device(t["d"], t["so"], t["sl"], 330, t["desc"], t["res"])
        W.batch_check_protocol_device(t["d"], t["so"], t["desc"], t["res"], 330, pres, EM, 0, 5, st, code)

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
        st.zero_()
        code.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        ecodes, eres, ewords = b.expect(EM, 0, 5, np.zeros(n, np.uint64))
        assert np.array_equal(code.cpu().numpy(), ecodes), kind
        assert np.array_equal(pres.cpu().numpy().view(P.RES_DTYPE), eres), kind
        assert np.array_equal(st.cpu().numpy().view(np.uint64), ewords), kind
        assert (eres["first_bad"] != P.NONE).any() == (kind == 2)
        assert lib.websocketframeGpuGetStat(b"workspace_bytes", C.byref(stat)) == 0
        held.append(stat.value)
    assert held[0] == held[1] > 0
    del g


# ------------------------------------------------------------------ 9: offsets past 4 GiB

def test_close_code_straddles_4gib(dev):
    """the CLOSE script's wire placed so that a masked CLOSE frame's two status bytes straddle arena
    offset 2^32 (its key just below): descriptors rebased, the arena's window and its low aliases
    unchanged"""
    H.need_memory(torch, pytest)
    b = PC.Batch(close_script(), 4, gap=5)
    d = b.desc[1 * 4 + 2]                                      # segment 1's CLOSE 0x3412
    assert int(d["type"]) == 8 and int(d["masked"]) == 1
    high = H.place(H.B32, int(d["data_off"]) + 1)
    arena = H.Arena(dev)
    img = b.raw[:-PC.PAD]
    placed = arena.put(high, img)
    state = np.zeros(b.nseg, np.uint64)
    exp = b.expect(WM, 0, 0, state)
    assert [int(c) for c in exp[1]["code"]] == [0, 7, 0, 7]
    lo, hi = H.window(high, len(img))
    check_call(dev, arena.view(high, len(img)), i64(dev, [o + high for o in b.seg_off]), up(dev, H.rebase(b.desc, high)),
               up(dev, b.res), b.nseg, 4, WM, 0, 0, state, exp, "2^32", window=(lo, hi))
    arena.check(placed, img, "2^32")
