"""websocketframeBatchHandshakeDevice (libwsframe_amd_hs.so) on the GPU, bit for bit against the
reference's recorded results (tests/golden/handshake_batch.json) and, for built requests, against
the host symbols of libwsframe_amd.so and the reference's own build where it is present
(handshake_cases.expected). Every call compares every output of every segment: the descriptor,
the 32 accept bytes, the response slot, and a sentinel fill that must be intact wherever nothing
is to be written; d_buf must come back unchanged.

Geometry: the parse kernel reads rounds of 64 lanes x 16 B from the segment's 16-B phase on, so
with segments placed at multiples of 16 a position p is lane (p % 1024) // 16, byte p % 16."""
import numpy as np
import pytest

import handshake_cases as HC
import wsynth
from oracle_lib import oracle_segments, used_descs
from util_amd import _lib
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT, ACC_SENT = 0x77, 0x5A


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.load_hs_lib()                                       # a missing library fails here, it never skips
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def expect():
    """expected values of a request: the host symbols', which must be the reference build's where
    that is present; computed once per distinct request"""
    host, ref, memo = HC.host_symbols(), HC.reference_lib(), {}

    def f(data):
        if data not in memo:
            memo[data] = HC.expected(host, data)
            if ref is not None:
                assert HC.expected(ref, data) == memo[data], data
        return memo[data]
    return f


def i64(dev, a):
    return torch.from_numpy(np.asarray(a, np.uint64).astype(np.int64)).to(dev)


def call(dev, buf, so, sl, flags=0, resp_cap=512, resp_off=None, want_resp=True, want_accept=True, resp_bytes=None):
    """one call on a packed batch; returns (records, accept [nseg, 32], response buffer), numpy"""
    nseg = len(so)
    d_buf = torch.from_numpy(buf).to(dev)
    before = d_buf.clone()
    hs = torch.full((max(1, nseg) * 32,), SENT, dtype=torch.uint8, device=dev)
    acc = torch.full((max(1, nseg) * 32,), ACC_SENT, dtype=torch.uint8, device=dev) if want_accept else None
    if resp_bytes is None:
        resp_bytes = nseg * resp_cap
    resp = torch.full((max(16, resp_bytes),), SENT, dtype=torch.uint8, device=dev) if want_resp else None
    W.batch_handshake_device(d_buf, i64(dev, so), i64(dev, sl), hs, flags, acc, resp,
                             None if resp_off is None else i64(dev, resp_off), resp_cap)
    torch.cuda.synchronize()
    assert torch.equal(d_buf, before), "d_buf modified"
    return (hs.cpu().numpy().view(W.HS_DTYPE)[:nseg], None if acc is None else acc.cpu().numpy().reshape(-1, 32)[:nseg],
            None if resp is None else resp.cpu().numpy())


def verify(reqs, exps, out, flags=0, resp_cap=512, resp_off=None, tag=""):
    recs, acc, resp = out
    want_resp = np.full(len(resp), SENT, np.uint8) if resp is not None else None
    for s, (d, x) in enumerate(zip(reqs, exps)):
        rec = tuple(int(v) for v in recs[s])
        want = HC.expected_record(x, flags, resp is not None, resp_cap)
        assert rec == want, "%s: segment %d (%d bytes) descriptor %s, expected %s" % (tag, s, len(d), rec, want)
        if acc is not None:
            wa = x["accept"] + b"\0\0\0\0" if x["ret"] > 0 else bytes([ACC_SENT]) * 32
            assert bytes(acc[s]) == wa, "%s: segment %d accept" % (tag, s)
        if resp is not None and want[6] == W.HS_RESP_WRITTEN:
            slot = int(resp_off[s]) if resp_off is not None else s * resp_cap
            r = x["resp_echo"] if flags & HC.ECHO else x["resp"]
            want_resp[slot:slot + len(r)] = np.frombuffer(r, np.uint8)
    if resp is not None:
        bad = np.nonzero(resp != want_resp)[0]
        assert not len(bad), "%s: response byte %d is %#x, expected %#x (%d differ)" % (
            tag, bad[0], resp[bad[0]], want_resp[bad[0]], len(bad))


def run(dev, expect, reqs, flags=0, resp_cap=512, align=16, bases=None, tag="", **kw):
    buf, so, sl = HC.pack(reqs, bases=bases, align=align)
    exps = [expect(r) for r in reqs]
    verify(reqs, exps, call(dev, buf, so, sl, flags, resp_cap, **kw), flags, resp_cap, kw.get("resp_off"), tag)
    return exps


# ------------------------------------------------------------------ the directed table (quirks)

@pytest.mark.parametrize("flags", [0, HC.ECHO])
def test_directed_table_against_the_fixture(dev, golden, flags):
    rows = golden("handshake_batch.json")
    table = HC.directed_table()
    assert [r["name"] for r in rows] == [n for n, _ in table]
    reqs = [d for _n, d in table]
    exps = [{"ret": r["ret"], "key_off": r["key_off"], "key_len": r["key_len"],
             "proto_off": HC.NONE if r["proto_off"] is None else r["proto_off"], "proto_len": r["proto_len"],
             "accept": r["accept"].encode(), "resp": bytes.fromhex(r["resp"]), "resp_echo": bytes.fromhex(r["resp_echo"])}
            for r in rows]
    for align in (16, 1):
        buf, so, sl = HC.pack(reqs, align=align)
        verify(reqs, exps, call(dev, buf, so, sl, flags, 512), flags, 512, tag="table, align %d" % align)


# ------------------------------------------------------------------ parse geometry

def test_terminator_at_every_offset(dev, expect):
    """the terminator starting at every offset 0..2100: every lane, every byte of a chunk, the
    chunk edges and two round edges"""
    reqs = [HC.terminator_at(o) for o in range(2101)]
    exps = run(dev, expect, reqs, HC.ECHO, 160, tag="terminator")
    assert all(x["ret"] == o + 4 or x["ret"] == -1 for o, x in enumerate(exps))
    assert sum(x["ret"] > 0 for x in exps) > 2000


def test_terminator_at_every_base(dev, expect):
    offs = (0, 1, 12, 13, 15, 16, 1008, 1020, 1021, 1023, 1024, 2047)
    for base in range(16):
        reqs = [HC.terminator_at(o) for o in offs]
        bases, pos = [], base
        for r in reqs:
            bases.append(pos)
            pos = (pos + len(r) + 47) // 16 * 16 + base
        run(dev, expect, reqs, 0, 144, bases=bases, tag="base %d" % base)


@pytest.mark.parametrize("which", [0, 1])
def test_pattern_at_every_offset(dev, expect, which):
    """the key (0) or protocol (1) pattern starting at every offset 0..1100: it straddles every
    chunk edge and the round edge"""
    reqs = [HC.pattern_at(o, which) for o in range(1101)]
    exps = run(dev, expect, reqs, HC.ECHO, 160, tag="pattern %d" % which)
    assert all(x["ret"] > 0 and x["proto_off"] != HC.NONE for x in exps)
    assert [x[("key_off", "proto_off")[which]] for x in exps] == [o + (19, 24)[which] for o in range(1101)]


@pytest.mark.parametrize("which", [0, 1])
def test_values_ending_at_a_round_edge(dev, expect, which):
    """values of 1..160 bytes whose end falls on the round edge (1024), one byte before and after
    it, and that straddle it by half"""
    reqs = [HC.value_ending_at(1024 + d, n, which) for n in range(1, 161) for d in (-1, 0, 1, n // 2)]
    exps = run(dev, expect, reqs, HC.ECHO, 320, tag="value %d" % which)
    assert [x[("key_len", "proto_len")[which]] for x in exps] == [n for n in range(1, 161) for _ in range(4)]


# ------------------------------------------------------------------ isolation

def test_bytes_outside_a_segment_do_not_count(dev, expect):
    """segments that end 1, 2 and 3 bytes into the terminator with the completing bytes right
    after them (the pad, which is the next segment's start), a terminator and a pattern completed
    only by pad bytes"""
    full = HC.request(proto=b"chat")
    reqs, gaps = [], []
    for cut in (1, 2, 3):
        reqs += [full[:-cut], full[-cut:] + full]            # adjacent: the next segment completes it
        gaps += [b"", b""]
    for cut in (1, 2, 3):
        reqs.append(full[:-cut])                             # the pad completes it
        gaps.append(full[-cut:] + b"\x81\x00")
    reqs.append(b"GET / HTTP/1.1\r\n\r\n" + HC.KEYPAT[:10])  # a pattern completed by pad bytes, after e
    gaps.append(HC.KEYPAT[10:] + b" " + HC.KEY + b"\r\n\r\n")
    reqs.append(b"GET / HTTP/1.1\r\n" + HC.KEYPAT + b" " + HC.KEY + b"\r\n" + HC.PROTOPAT[:22])
    gaps.append(b": chat\r\n\r\n")                           # pattern and terminator only in the pad
    bases, pos = [], 5
    for r, g in zip(reqs, gaps):
        bases.append(pos)
        pos += len(r) + (len(g) + 40 if g else 0)
    buf, so, sl = HC.pack(reqs, bases=bases)
    for b, r, g in zip(bases, reqs, gaps):
        buf[b + len(r):b + len(r) + len(g)] = np.frombuffer(g, np.uint8)
    exps = [expect(r) for r in reqs]
    assert [x["ret"] for x in exps] == [0, 107, 0, 108, 0, 109, 0, 0, 0, -1, 0]
    for flags in (0, HC.ECHO):
        verify(reqs, exps, call(dev, buf, so, sl, flags, 192), flags, 192, tag="isolation")


# ------------------------------------------------------------------ SHA-1

def test_every_key_length(dev, expect):
    """keys of 1..160 bytes through the parse: every padding position and the block-count steps
    (19/20, 27/28, 83/84, 91/92); accept and response compared"""
    reqs = [HC.request(key=HC.filler(n, n), proto=b"p%d" % n) for n in range(1, 161)]
    exps = run(dev, expect, reqs, HC.ECHO, 176, align=1, tag="key length")
    assert [x["key_len"] for x in exps] == list(range(1, 161))
    assert all(n in range(1, 161) for n in HC.KEY_STEPS)


# ------------------------------------------------------------------ packing

@pytest.fixture(scope="module")
def mixed():
    return HC.random_requests(600, seed=11)


@pytest.mark.parametrize("nseg", [1, 63, 64, 65, 257])
def test_segment_counts_with_mixed_classes(dev, expect, mixed, nseg):
    reqs = list(mixed[:nseg])
    if nseg > 2:
        reqs[1] = b""                                        # empty segments
        reqs[nseg // 2] = b""
    exps = run(dev, expect, reqs, HC.ECHO, 224, align=1, tag="nseg %d" % nseg)
    if nseg >= 63:
        assert {x["ret"] > 0 for x in exps[:64]} == {True, False}    # classes mixed inside one wave
        assert {x["ret"] for x in exps} >= {0, -1}


def test_response_offsets_with_unaligned_slots(dev, expect, mixed):
    reqs = mixed[:130]
    cap = 208
    off = [s * 240 + (s % 16) for s in range(len(reqs))]    # every 16-B phase, dword-aligned ones included
    for flags in (0, HC.ECHO):
        run(dev, expect, reqs, flags, cap, align=1, resp_off=off, resp_bytes=off[-1] + cap + 16, tag="resp_off")


def test_response_capacity_edges(dev, expect):
    req = HC.request(proto=b"chat")
    x = expect(req)
    assert len(x["resp"]) == 129 and len(x["resp_echo"]) == 155 + 4
    for flags, caps in ((0, (128, 129, 130)), (HC.ECHO, (154 + 4, 155 + 4, 156 + 4))):
        for cap in caps:
            reqs = [req, HC.request(), req]
            buf, so, sl = HC.pack(reqs, align=16)
            out = call(dev, buf, so, sl, flags, cap)
            verify(reqs, [expect(r) for r in reqs], out, flags, cap, tag="cap %d" % cap)
            assert int(out[0][0]["flags"]) == (W.HS_RESP_NO_SPACE if cap == caps[0] else W.HS_RESP_WRITTEN)
            assert int(out[0][0]["resp_len"]) == caps[1]


def test_optional_outputs(dev, expect, mixed):
    reqs = mixed[:70]
    run(dev, expect, reqs, HC.ECHO, 0, align=1, want_resp=False, tag="no resp")
    run(dev, expect, reqs, HC.ECHO, 224, align=1, want_accept=False, tag="no accept")
    run(dev, expect, reqs, 0, 0, align=1, want_resp=False, want_accept=False, tag="parse only")


# ------------------------------------------------------------------ arguments

def test_arguments(dev, expect):
    lib = _lib.load_hs_lib()
    req = HC.request()
    buf, so, sl = HC.pack([req, req], align=16)
    d_buf = torch.from_numpy(buf).to(dev)
    hs = torch.full((3 * 32,), SENT, dtype=torch.uint8, device=dev)
    for flags in (2, 3, 0x80000000):
        with pytest.raises(RuntimeError):
            W.batch_handshake_device(d_buf, i64(dev, so), i64(dev, sl), hs, flags)
        assert lib.websocketframeGpuLastError() != b""
    W.batch_handshake_device(d_buf, i64(dev, so[:0]), i64(dev, sl[:0]), hs)          # nseg 0: a no-op
    torch.cuda.synchronize()
    assert (hs == SENT).all()
    # a hand-built length of 2^31 (buflen to match) and a segment past buflen: flagged, never read;
    # the segment between them is served as usual
    so3 = np.array([0, so[1], 1 << 40], np.uint64)
    sl3 = np.array([1 << 31, sl[1], 10], np.uint64)
    acc = torch.full((3 * 32,), ACC_SENT, dtype=torch.uint8, device=dev)
    resp = torch.full((3 * 144,), SENT, dtype=torch.uint8, device=dev)
    W.batch_handshake_device(d_buf, i64(dev, so3), i64(dev, sl3), hs, 0, acc, resp, None, 144, buflen=(1 << 31) + 64)
    torch.cuda.synchronize()
    recs = hs.cpu().numpy().view(W.HS_DTYPE)
    x = expect(req)
    for s in (0, 2):
        assert tuple(int(v) for v in recs[s]) == (-1, 0, 0, W.HS_NONE, 0, 0, W.HS_ERR_SEG_LEN, 0)
    assert tuple(int(v) for v in recs[1]) == HC.expected_record(x, 0, True, 144)
    r = resp.cpu().numpy()
    assert (r[:144] == SENT).all() and (r[288:] == SENT).all() and bytes(r[144:144 + 129]) == x["resp"]
    a = acc.cpu().numpy()
    assert (a[:32] == ACC_SENT).all() and (a[64:] == ACC_SENT).all() and bytes(a[32:60]) == x["accept"]


# ------------------------------------------------------------------ seeded random

def test_seeded_random_batch(dev, expect):
    """4,096 requests of 20..3,000 bytes in one batch (the requests whose coverage
    tests/test_handshake_host.py asserts)"""
    reqs = HC.random_requests()
    for flags, align in ((HC.ECHO, 1), (0, 16)):
        run(dev, expect, reqs, flags, 224, align=align, tag="random, align %d" % align)


# ------------------------------------------------------------------ captured

def test_captured_call_follows_the_bytes(dev, expect):
    """one warm call, then a capture; replayed after rewriting the request bytes (same segment
    table), the results follow the bytes"""
    a = [HC.request(key=HC.filler(24, s), proto=b"chat") for s in range(100)]
    b = [(HC.request(key=HC.filler(24, s), proto=b"chat").replace(b"Sec-WebSocket-Key", b"Sec-WebSocket-key"),
          HC.request(key=HC.filler(24, s), proto=b"chat")[:-1] + b"X",
          HC.request(key=HC.filler(24, s + 7), proto=b"chat"))[s % 3] for s in range(100)]
    assert [len(r) for r in a] == [len(r) for r in b]
    buf_a, so, sl = HC.pack(a, align=1)
    buf_b, _so, _sl = HC.pack(b, align=1)
    d_buf = torch.from_numpy(buf_a).to(dev)
    d_so, d_sl = i64(dev, so), i64(dev, sl)
    hs = torch.zeros(100 * 32, dtype=torch.uint8, device=dev)
    acc = torch.zeros(100 * 32, dtype=torch.uint8, device=dev)
    resp = torch.zeros(100 * 176, dtype=torch.uint8, device=dev)

    def once():
        W.batch_handshake_device(d_buf, d_so, d_sl, hs, HC.ECHO, acc, resp, None, 176)

    once()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        once()
    for reqs, wire in ((b, buf_b), (a, buf_a), (b, buf_b)):
        d_buf.copy_(torch.from_numpy(wire).to(dev))
        hs.fill_(SENT)
        acc.fill_(ACC_SENT)
        resp.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        out = (hs.cpu().numpy().view(W.HS_DTYPE), acc.cpu().numpy().reshape(-1, 32), resp.cpu().numpy())
        verify(reqs, [expect(r) for r in reqs], out, HC.ECHO, 176, tag="replay")
    assert {expect(r)["ret"] > 0 for r in b} == {True, False}


# ------------------------------------------------------------------ handover to the decode

def test_frames_after_the_request_decode_as_the_oracle_says(dev, expect):
    """a request followed by masked frames in the same inbuf: after the handshake call, a batch
    decode over [seg_off + ret, seg_off + seg_len) equals the oracle's decode of those bytes"""
    inbufs = []
    for s in range(9):
        wire, off, _pl, _plain = wsynth.make_batch(3 + s, wsynth.PLEN_MIX3, 0, wsynth.B0_BINARY, 100 + s)
        wire = np.concatenate([wire, wire[:s]])                               # + an incomplete tail
        inbufs.append(HC.request(key=HC.filler(24, s), proto=b"chat" if s % 2 else None) + wire.tobytes())
    buf, so, sl = HC.pack(inbufs, align=1)
    exps = [expect(r) for r in inbufs]
    out = call(dev, buf, so, sl, HC.ECHO, 176)
    verify(inbufs, exps, out, HC.ECHO, 176, tag="handover")
    ret = out[0]["ret"].astype(np.uint64)
    assert (out[0]["ret"] > 0).all()
    fo, fl = so + ret, sl - ret
    d = torch.from_numpy(buf).to(dev)
    mf = 16
    desc = torch.zeros(len(so) * mf * 32, dtype=torch.uint8, device=dev)
    res = torch.zeros(len(so) * 16, dtype=torch.uint8, device=dev)
    W.batch_decode_device(d, i64(dev, fo), i64(dev, fl), mf, desc, res)
    torch.cuda.synchronize()
    ob = buf.copy()
    od, orr = oracle_segments(ob, [int(v) for v in fo], [int(v) for v in fl], mf)
    gd, gr = desc.cpu().numpy().view(W.DESC_DTYPE), res.cpu().numpy().view(W.SEGRES_DTYPE)
    assert np.array_equal(d.cpu().numpy(), ob), "payload bytes differ from the oracle"
    assert np.array_equal(gr, orr) and np.array_equal(used_descs(gd, gr, mf), used_descs(od, orr, mf))
    assert all(int(n) >= 3 + s for s, n in enumerate(gr["n_frames"]))
