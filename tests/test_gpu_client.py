"""websocketframeBatchClientRequestDevice and websocketframeBatchClientVerifyDevice
(libwsframe_amd_cli.so) on the GPU, bit for bit against the model of tests/client_oracle.py. Every
call compares every output of every segment, with a sentinel fill that must be intact wherever
nothing is to be written; d_buf must come back unchanged.

Geometry: the verify kernel reads rounds of 64 lanes x 16 B from the segment's 16-B phase on, so
with segments placed at multiples of 16 a position p is lane (p % 1024) // 16, byte p % 16."""
import numpy as np
import pytest

import client_cases as CC
import client_oracle as CO
import handshake_cases as HC
import wsynth
from oracle_lib import oracle_segments, used_descs
from util_amd import _lib
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT, EXP_SENT = 0x77, 0x5A


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.load_cli_lib()                                      # a missing library fails here, it never skips
    return torch.device("cuda:0")


def i64(dev, a):
    return torch.from_numpy(np.asarray(a, np.uint64).astype(np.int64)).to(dev)


def u8(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def verify_call(dev, buf, so, sl, expects, offered=None, max_head=0):
    """one verify call on a packed batch; expects: one 32-byte value or a list of them; offered: None
    (no entries) or a list of offered lists. Returns the records as tuples."""
    nseg = len(so)
    d_buf = torch.from_numpy(buf).to(dev)
    before = d_buf.clone()
    if isinstance(expects, bytes):
        expects = [expects] * nseg
    d_exp = u8(dev, np.frombuffer(b"".join(expects) + b"\0" * 32, np.uint8))
    cv = torch.full((max(1, nseg) * 32,), SENT, dtype=torch.uint8, device=dev)
    strs = entry = None
    if offered is not None:
        p, ent = CC.pool([(b"/", o, b"") for o in offered])
        strs, entry = u8(dev, p), u8(dev, ent)
    W.batch_client_verify_device(d_buf, i64(dev, so), i64(dev, sl), d_exp, cv, strs, entry, max_head)
    torch.cuda.synchronize()
    assert torch.equal(d_buf, before), "d_buf modified"
    return [tuple(int(v) for v in r) for r in cv.cpu().numpy().view(W.CLI_VERIFY_DTYPE)[:nseg]]


def check(dev, cases, max_head=0, align=16, bases=None, tag="", expects=CC.EXPECT, entries=True, gaps=None):
    """cases: (data, offered) pairs; the whole batch against the model"""
    segs = [d for d, _o in cases]
    buf, so, sl = CC.pack(segs, bases=bases, align=align)
    for b, r, g in zip(so, segs, gaps or ()):
        buf[int(b) + len(r):int(b) + len(r) + len(g)] = np.frombuffer(g, np.uint8)
    got = verify_call(dev, buf, so, sl, expects, [o for _d, o in cases] if entries else None, max_head)
    ex = [expects] * len(cases) if isinstance(expects, bytes) else expects
    want = [CO.verify(d, e, o if entries else b"", max_head) for (d, o), e in zip(cases, ex)]
    for s, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: segment %d (%d bytes, max_head %d) is %s, the model says %s" % (tag, s, len(segs[s]), max_head, g, w)
    return want


# ------------------------------------------------------------------ the directed table

def test_directed_table(dev):
    """the whole table in one batch, under each max_head that a row names (0 among them), at two
    alignments"""
    table = CC.directed_table()
    cases = [(d, o) for _n, d, o, _m in table]
    seen = set()
    for max_head in sorted({m for _n, _d, _o, m in table}):
        for align in (16, 1):
            want = check(dev, cases, max_head, align, tag="table, max_head %d, align %d" % (max_head, align))
            if max_head == 0:
                seen |= {CO.result_class(w) for w in want}
            else:
                seen |= {CO.result_class(w) for w in want if w[1] == CO.TOO_LONG}
    assert seen == set(CC.CLASSES)


# ------------------------------------------------------------------ geometry

def test_terminator_at_every_offset(dev):
    """the terminator starting at every offset 1000..1060: the last lanes of a round, the round edge,
    every byte of a chunk; "\\r\\n" split over a chunk edge (15 | 16) and the round edge (1023 | 1024)"""
    offs = list(range(1000, 1061))
    cases = [(CC.terminator_at(o), b"") for o in offs]
    assert {1007, 1008, 1022, 1023, 1024} <= set(offs)       # "\r\n" and "\r\n\r\n" astride chunk and round edges
    want = check(dev, cases, tag="terminator")
    assert [w[0] for w in want] == [o + 4 for o in offs]
    for mh in (1024, 1028, 1030):
        check(dev, cases, mh, tag="terminator, max_head %d" % mh)


def test_terminator_at_every_base(dev):
    offs = (1000, 1007, 1008, 1020, 1021, 1023, 1024, 1039)
    for base in range(16):
        cases = [(CC.terminator_at(o), b"") for o in offs]
        bases, pos = [], base
        for d, _o in cases:
            bases.append(pos)
            pos = (pos + len(d) + 47) // 16 * 16 + base
        want = check(dev, cases, bases=bases, tag="base %d" % base)
        assert all(w[0] > 0 for w in want)


def test_header_at_every_offset(dev):
    """each of the five names starting at every offset 1000..1050 (name and value cross the round
    edge), values padded with 0..130 bytes of SP and HT"""
    cases = CC.header_cases()
    want = check(dev, cases, tag="header position")
    assert all(w[0] > 0 and w[3] != CO.NONE and w[4] == 4 for w in want)


# ------------------------------------------------------------------ isolation

def test_bytes_outside_a_segment_do_not_count(dev):
    """bytes after a segment that would complete the terminator, a header name or the 28th accept
    byte, and a neighbour segment that holds the right Accept line: none counts. The next segment
    starts 0 and 1..31 bytes after each; the completing bytes fill the gap and run on into it."""
    g = CC.good()
    no_acc = CC.good(acc=None)
    cut_name = CC.resp([CC.STATUS_LINE, CC.UP, CC.CONN])[:-4] + b"\r\nSec-WebSocket-Acc"
    rows = [(g[:-1], g[-1:]), (g[:-2], g[-2:]), (g[:-3], g[-3:]), (cut_name, b"ept: " + CC.ACC + b"\r\n\r\n"),
            (g[:-5], g[-5:]), (no_acc, CC.ACCEPT_NAME + CC.ACC + b"\r\n\r\n")]
    assert CO.verify(no_acc, CC.EXPECT)[:2] == (-1, CO.ACCEPT) and g[:-5].endswith(CC.ACC[:27])
    for gap in (0, 1, 2, 3, 15, 16, 17, 31):
        cases, gaps, bases, pos = [], [], [], 3
        for seg, after in rows:
            nxt = after[gap:] + g                             # the neighbour: what is left of the completing bytes, then its own
            for d, fill in ((seg, after[:gap]), (nxt, b"")):
                cases.append((d, b""))
                gaps.append(fill)
                bases.append(pos)
                pos += len(d) + (gap if d is seg else 37)
        want = check(dev, cases, bases=bases, gaps=gaps, tag="isolation, gap %d" % gap)
        assert all(w[0] <= 0 for w in want[::2]) and [w[0] for w in want[:6:2]] == [0, 0, 0]
        assert want[10][:2] == (-1, CO.ACCEPT)


# ------------------------------------------------------------------ packing

@pytest.fixture(scope="module")
def mixed():
    return [(d, o) for d, o, m in CC.random_responses(900, seed=11) if m == 0][:300]


@pytest.mark.parametrize("nseg", [1, 63, 64, 65, 257])
def test_segment_counts_with_mixed_classes(dev, mixed, nseg):
    cases = list(mixed[:nseg])
    if nseg > 2:
        cases[1] = (b"", b"")
        cases[nseg // 2] = (b"", b"chat")
    want = check(dev, cases, align=1, tag="nseg %d" % nseg)
    if nseg >= 63:
        assert len({CO.result_class(w) for w in want}) >= 8


def test_seeded_sweep(dev):
    """the 4,096 responses whose coverage tests/test_client_host.py asserts, by their max_head"""
    cases = CC.random_responses()
    zero = [(d, o) for d, o, m in cases if m == 0]
    check(dev, zero, align=1, tag="sweep")
    check(dev, zero, align=16, tag="sweep, aligned", entries=False)
    rest = [(d, o, m) for d, o, m in cases if m]
    for mh in sorted({m for _d, _o, m in rest})[::16]:
        check(dev, [(d, o) for d, o, m in rest if m == mh], mh, align=1, tag="sweep, max_head %d" % mh)
    by_class = {}
    for d, o, m in rest:
        by_class.setdefault(m % 7, []).append((d, o))
    for k, group in by_class.items():
        check(dev, group, 700 + k, align=1, tag="sweep under max_head %d" % (700 + k))


# ------------------------------------------------------------------ the request call

def request_call(dev, strings, nonces, req_cap, req_off=None, req_bytes=None, want_req=True, ent=None, strs=None):
    n = len(strings)
    p, e = CC.pool(strings)
    if ent is not None:
        e = ent
    d_str = u8(dev, p if strs is None else strs)
    d_ent = u8(dev, e)
    d_nonce = u8(dev, np.frombuffer(b"".join(nonces), np.uint8))
    if req_bytes is None:
        req_bytes = n * req_cap
    req = torch.full((max(16, req_bytes),), SENT, dtype=torch.uint8, device=dev) if want_req else None
    expect = torch.full((n * 32,), EXP_SENT, dtype=torch.uint8, device=dev)
    rd = torch.full((n * 16,), SENT, dtype=torch.uint8, device=dev)
    W.batch_client_request_device(d_str, d_ent, d_nonce, req, expect, rd, None if req_off is None else i64(dev, req_off), req_cap)
    torch.cuda.synchronize()
    return (rd.cpu().numpy().view(W.CLI_REQ_DTYPE), None if req is None else req.cpu().numpy(), expect.cpu().numpy().reshape(n, 32))


def check_request(strings, nonces, out, req_cap, req_off=None, in_range=None, tag=""):
    rd, req, expect = out
    want_req = np.full(len(req), SENT, np.uint8) if req is not None else None
    for s, ((path, proto, host), nonce) in enumerate(zip(strings, nonces)):
        rec, text, exp = CO.request_record(path, nonce, proto, host, req_cap if req is not None else None,
                                           True if in_range is None else in_range[s])
        assert tuple(int(v) for v in rd[s]) == rec, "%s: connection %d descriptor" % (tag, s)
        assert bytes(expect[s]) == (exp if exp is not None else bytes([EXP_SENT]) * 32), "%s: connection %d expect" % (tag, s)
        if text is not None:
            slot = int(req_off[s]) if req_off is not None else s * req_cap
            want_req[slot:slot + len(text)] = np.frombuffer(text, np.uint8)
    if req is not None:
        bad = np.nonzero(req != want_req)[0]
        assert not len(bad), "%s: request byte %d is %#x, expected %#x (%d differ)" % (
            tag, bad[0], req[bad[0]], want_req[bad[0]], len(bad))


def conn_strings(n):
    out = []
    for s in range(n):
        path = b"/" + HC.filler(s % 41, s)
        out.append((path, (b"", b"chat", b"a, bb ,ccc")[s % 3], (b"", b"h%d.example.com" % s)[s % 2]))
    return out


def nonces(n, salt=0):
    return [bytes((s * 37 + k * 11 + salt) & 0xFF for k in range(16)) for s in range(n)]


@pytest.mark.parametrize("nseg", [1, 63, 64, 65, 257])
def test_request_segment_counts(dev, nseg):
    strings, nn = conn_strings(nseg), nonces(nseg)
    check_request(strings, nn, request_call(dev, strings, nn, 256), 256, tag="request nseg %d" % nseg)


def test_request_slots_at_unaligned_offsets(dev):
    strings, nn = conn_strings(130), nonces(130, 3)
    cap = 224
    off = [s * 256 + (s % 16) + (s // 16 % 2) * 4 for s in range(130)]        # every 16-B phase
    out = request_call(dev, strings, nn, cap, off, off[-1] + cap + 16)
    check_request(strings, nn, out, cap, off, tag="req_off")


def test_request_capacity_edges_and_optional_buffer(dev):
    strings, nn = [(b"/chat", b"chat", b"example.com")] * 3 + [(b"/", b"", b"")], nonces(4)
    n0 = len(CO.request(*strings[0][:1], nn[0], strings[0][1], strings[0][2]))
    for cap, fl in ((n0 - 1, W.CLI_REQ_NO_SPACE), (n0, W.CLI_REQ_WRITTEN), (n0 + 1, W.CLI_REQ_WRITTEN)):
        out = request_call(dev, strings, nn, cap)
        check_request(strings, nn, out, cap, tag="cap %d" % cap)
        assert int(out[0][0]["flags"]) == fl and int(out[0][0]["req_len"]) == n0 and int(out[0][3]["flags"]) == W.CLI_REQ_WRITTEN
    out = request_call(dev, strings, nn, 0, want_req=False)
    check_request(strings, nn, out, 0, tag="no request buffer")


def test_request_error_flags(dev):
    """every error flag; nothing is written for those connections: no request and no d_expect"""
    strings = [(b"/ok", b"chat", b"h"), (b"/a b", b"", b""), (b"/a", b"x\r\ny", b""), (b"/a", b"", b"h\x7f"), (b"/\x01", b"", b""),
               (b"/ok2", b"", b""), (b"/r1", b"", b""), (b"/r2", b"p", b""), (b"/r3", b"", b"h"), (b"/last", b"a b", b"h h")]
    nn = nonces(len(strings))
    p, ent = CC.pool(strings)
    in_range = [True] * len(strings)
    ent[6]["path_off"], in_range[6] = len(p) - 1, False                          # path_len 3 passes the pool's end
    ent[7]["proto_off"], in_range[7] = 1 << 40, False
    ent[8]["host_len"], in_range[8] = 0xFFFFFFFF, False
    out = request_call(dev, strings, nn, 192, ent=ent, strs=p)
    check_request(strings, nn, out, 192, in_range=in_range, tag="errors")
    fl = [int(f) for f in out[0]["flags"]]
    assert fl == [1, 8, 8, 8, 8, 1, 4, 4, 4, 1]
    ent2 = ent.copy()
    ent2[0]["path_len"] = 0                                                       # an empty path
    out = request_call(dev, strings, nn, 192, ent=ent2, strs=p)
    assert int(out[0][0]["flags"]) == W.CLI_ERR_RANGE and (out[2][0] == EXP_SENT).all() and (out[1][:192] == SENT).all()


# ------------------------------------------------------------------ arguments

def test_arguments(dev):
    lib = _lib.load_cli_lib()
    g = CC.good()
    buf, so, sl = CC.pack([g, g], align=16)
    d_buf = torch.from_numpy(buf).to(dev)
    d_exp = u8(dev, np.frombuffer(CC.EXPECT * 3, np.uint8))
    cv = torch.full((3 * 32,), SENT, dtype=torch.uint8, device=dev)
    strings, nn = conn_strings(2), nonces(2)
    p, ent = CC.pool(strings)
    d_str, d_ent, d_nonce = u8(dev, p), u8(dev, ent), u8(dev, np.frombuffer(b"".join(nn), np.uint8))
    req = torch.full((512,), SENT, dtype=torch.uint8, device=dev)
    rd = torch.full((32,), SENT, dtype=torch.uint8, device=dev)
    ex = torch.full((64,), EXP_SENT, dtype=torch.uint8, device=dev)
    for flags in (1, 2, 0x80000000):
        with pytest.raises(RuntimeError):
            W.batch_client_verify_device(d_buf, i64(dev, so), i64(dev, sl), d_exp, cv, flags=flags)
        assert lib.websocketframeGpuLastError() != b""
        with pytest.raises(RuntimeError):
            W.batch_client_request_device(d_str, d_ent, d_nonce, req, ex, rd, None, 256, flags=flags)
    W.batch_client_verify_device(d_buf, i64(dev, so[:0]), i64(dev, sl[:0]), d_exp, cv)            # nseg 0: no-ops
    W.batch_client_request_device(d_str, d_ent[:0], d_nonce, req, ex, rd, None, 256)
    torch.cuda.synchronize()
    assert (cv == SENT).all() and (req == SENT).all() and (rd == SENT).all() and (ex == EXP_SENT).all()
    # a hand-built length of 2^31 (buflen to match) and a segment past buflen: flagged, never read;
    # the segment between them is served as usual
    so3 = np.array([0, so[1], 1 << 40], np.uint64)
    sl3 = np.array([1 << 31, sl[1], 10], np.uint64)
    W.batch_client_verify_device(d_buf, i64(dev, so3), i64(dev, sl3), d_exp, cv, buflen=(1 << 31) + 64)
    torch.cuda.synchronize()
    recs = [tuple(int(v) for v in r) for r in cv.cpu().numpy().view(W.CLI_VERIFY_DTYPE)]
    assert recs[0] == recs[2] == (-1, 0, 0, W.CLI_NONE, 0, W.CLI_NONE, W.CLI_ERR_SEG_LEN, 0)
    assert recs[1] == CO.verify(g, CC.EXPECT)


def test_verify_without_entries(dev):
    """d_entry NULL: nothing was offered, so a protocol header fails; everything else as with them"""
    table = CC.directed_table()
    want = check(dev, [(d, o) for _n, d, o, _m in table], entries=False, tag="no entries")
    assert CO.PROTOCOL in {w[1] for w in want}


# ------------------------------------------------------------------ captured

def test_captured_calls_follow_the_bytes(dev):
    """both calls captured once in one graph on one stream; replayed after the nonces and the
    response bytes change, the results follow the bytes"""
    n = 100
    strings = conn_strings(n)
    p, ent = CC.pool(strings)
    d_str, d_ent = u8(dev, p), u8(dev, ent)
    d_nonce = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    req = torch.zeros(n * 256, dtype=torch.uint8, device=dev)
    expect = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    rd = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    cv = torch.zeros(n * 32, dtype=torch.uint8, device=dev)

    def responses(nn, variant):
        out = []
        for s in range(n):
            acc = CO.expect_of(nn[s])[:28]
            kind = (s + variant) % 3
            out.append(CC.good(acc=acc) if kind == 0 else (CC.good(acc=acc[::-1]) if kind == 1 else CC.good(acc=acc, up=b"Upgrade: Websocket")))
        return out

    nn_a, nn_b = nonces(n, 1), nonces(n, 2)
    buf0, so, sl = CC.pack(responses(nn_a, 0), align=1)
    d_buf = torch.from_numpy(buf0).to(dev)
    d_so, d_sl = i64(dev, so), i64(dev, sl)

    def once():
        W.batch_client_request_device(d_str, d_ent, d_nonce, req, expect, rd, None, 256)
        W.batch_client_verify_device(d_buf, d_so, d_sl, expect, cv, d_str, d_ent)

    once()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        once()
    for nn, variant in ((nn_b, 1), (nn_a, 0), (nn_b, 2)):
        rs = responses(nn, variant)
        wire, so2, _sl = CC.pack(rs, align=1)
        assert np.array_equal(so2, so)
        d_buf.copy_(torch.from_numpy(wire).to(dev))
        d_nonce.copy_(u8(dev, np.frombuffer(b"".join(nn), np.uint8)))
        for t, v in ((req, SENT), (expect, EXP_SENT), (rd, SENT), (cv, SENT)):
            t.fill_(v)
        g.replay()
        torch.cuda.synchronize()
        check_request(strings, nn, (rd.cpu().numpy().view(W.CLI_REQ_DTYPE), req.cpu().numpy(), expect.cpu().numpy().reshape(n, 32)),
                      256, tag="replay")
        got = [tuple(int(v) for v in r) for r in cv.cpu().numpy().view(W.CLI_VERIFY_DTYPE)]
        want = [CO.verify(r, CO.expect_of(x), st[1]) for r, x, st in zip(rs, nn, strings)]
        assert got == want
        assert {w[0] > 0 for w in want} == {True, False}


# ------------------------------------------------------------------ end to end on the device

def test_request_to_server_to_verify_to_decode(dev):
    """the request call's output into websocketframeBatchHandshakeDevice, its d_resp into the verify
    call: all ok; then frames appended after each response decode from ret on exactly as the oracle
    says"""
    n = 9
    strings = [(b"/chat/%d" % s, (b"", b"chat")[s % 2], (b"", b"example.com")[s % 3 == 0]) for s in range(n)]
    nn = nonces(n, 9)
    cap = 256
    rd, req, expect = request_call(dev, strings, nn, cap)
    check_request(strings, nn, (rd, req, expect), cap, tag="end to end")
    # the requests as the server's rx batch (slot s at s * cap; the slack after each is the pad)
    d_req = torch.from_numpy(np.concatenate([req, np.zeros(W.BATCH_PAD, np.uint8)])).to(dev)
    so = np.arange(n, dtype=np.uint64) * cap
    sl = rd["req_len"].astype(np.uint64)
    hs = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    acc = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    rcap = 192
    resp = torch.zeros(n * rcap, dtype=torch.uint8, device=dev)
    W.batch_handshake_device(d_req, i64(dev, so), i64(dev, sl), hs, W.HS_ECHO_PROTOCOL, acc, resp, None, rcap)
    torch.cuda.synchronize()
    h = hs.cpu().numpy().view(W.HS_DTYPE)
    assert (h["ret"] == rd["req_len"]).all() and (h["flags"] == W.HS_RESP_WRITTEN).all()
    assert np.array_equal(acc.cpu().numpy().reshape(n, 32), expect)
    r = resp.cpu().numpy().reshape(n, rcap)
    inbufs = []
    for s in range(n):
        wire, _off, _pl, _plain = wsynth.make_batch(3 + s, wsynth.PLEN_MIX3, 0, wsynth.B0_BINARY, 200 + s)
        wire = np.concatenate([wire, wire[:s]])                                   # + an incomplete tail
        inbufs.append(bytes(r[s][:int(h["resp_len"][s])]) + wire.tobytes())
    buf, so2, sl2 = CC.pack(inbufs, align=1)
    exps = [bytes(e) for e in expect]
    got = verify_call(dev, buf, so2, sl2, exps, [st[1] for st in strings])
    want = [CO.verify(d, e, st[1]) for d, e, st in zip(inbufs, exps, strings)]
    assert got == want and all(g[0] == int(h["resp_len"][s]) for s, g in enumerate(got))
    assert [g[4] for g in got] == [len(st[1]) for st in strings]
    ret = np.array([g[0] for g in got], np.uint64)
    fo, fl = so2 + ret, sl2 - ret
    d = torch.from_numpy(buf).to(dev)
    mf = 16
    desc = torch.zeros(n * mf * 32, dtype=torch.uint8, device=dev)
    res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    W.batch_decode_device(d, i64(dev, fo), i64(dev, fl), mf, desc, res)
    torch.cuda.synchronize()
    ob = buf.copy()
    od, orr = oracle_segments(ob, [int(v) for v in fo], [int(v) for v in fl], mf)
    gd, gr = desc.cpu().numpy().view(W.DESC_DTYPE), res.cpu().numpy().view(W.SEGRES_DTYPE)
    assert np.array_equal(d.cpu().numpy(), ob), "payload bytes differ from the oracle"
    assert np.array_equal(gr, orr) and np.array_equal(used_descs(gd, gr, mf), used_descs(od, orr, mf))
    assert all(int(k) >= 3 + s for s, k in enumerate(gr["n_frames"]))
