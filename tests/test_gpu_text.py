"""websocketframeBatchValidateTextDevice (libwsframe_amd_text.so) on the GPU against the oracle
(text_oracle.py: CPython's strict decoder over each connection's bytes so far): verdicts,
first_bad and the exact state word, on hand-built reassembly outputs, across batches, behind
the three reassembly entry points, on random text, on one large message and inside a captured
graph. Every call also checks that verdict slots past d_nmsg keep a sentinel and that d_out,
d_msg and d_desc come back byte-identical."""
import ctypes as C

import numpy as np
import pytest

import reasm_cases as R
import text_oracle as T
from oracle_lib import oracle_reassemble
from reasm_ctl_oracle import oracle_reassemble_ctl, region_image
from util_amd import _lib
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0x5A5A5A5A
POISON = (0xFF, 0xC2, 0xF0)
CHUNK, ROW, TILE = W.TEXT_CHUNK, W.TEXT_ROW, W.TEXT_TILE     # the kernel's 16-B chunk, 64-lane row and tile
SEQS = {2: b"\xc2\xa2", 3: b"\xe2\x82\xac", 4: b"\xf0\x90\x8d\x88"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.load_text_lib()                                     # a missing library fails here, it never skips
    return torch.device("cuda:0")


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def validate(dev, out, desc, msg, nmsg, mf, state, conns, segs, tag="", out_window=None):
    """one validator call on device tensors; segs[s] = the oracle's view of segment s's listed
    messages [(opcode, body, complete, continued, n_frames)]; conns[s] its TextConn. Compares
    everything the call writes and everything it must not write (of d_out the bytes
    [out_window[0], out_window[1]) where one is given: an arena is never copied as a whole)."""
    nseg = len(segs)
    verdict = torch.full((nseg * mf,), SENTINEL, dtype=torch.int32, device=dev)
    first_bad = torch.full((nseg,), SENTINEL, dtype=torch.int32, device=dev)
    seen = out if out_window is None else out[out_window[0]:out_window[1]]
    before = [t.clone() for t in (seen, desc, msg)]
    st_in = None if state is None else u32(state).copy()
    W.batch_validate_text_device(out, desc, msg, nmsg, mf, verdict, text_state=state, first_bad=first_bad)
    torch.cuda.synchronize()
    for t, b, name in zip((seen, desc, msg), before, ("d_out", "d_desc", "d_msg")):
        assert torch.equal(t, b), "%s %s modified" % (tag, name)
    gv, gf = u32(verdict).reshape(nseg, mf), u32(first_bad)
    gs = None if state is None else u32(state)
    for s in range(nseg):
        ov, ofb, oword = conns[s].batch(segs[s])
        n = len(segs[s])
        assert list(gv[s, :n]) == ov, "%s segment %d verdicts %s, oracle %s" % (tag, s, list(gv[s, :n]), ov)
        assert (gv[s, n:] == SENTINEL).all(), "%s segment %d: verdict slots past d_nmsg written" % (tag, s)
        assert int(gf[s]) == ofb, "%s segment %d first_bad %d, oracle %d" % (tag, s, gf[s], ofb)
        if gs is not None:
            assert int(gs[s]) == oword, "%s segment %d state %08x -> %08x, oracle %08x" % (tag, s, st_in[s], gs[s], oword)
    return gv


def direct(dev, segs, mf, conns=None, state=None, phases=None, tag="", arena=None, base=0):
    """hand-built d_out / d_msg / d_desc: message i of a segment takes frame slot i; bodies are
    laid out one after the other, each at its 16-B phase (phases[s][i], default cycling), with
    0xFF / 0xC2 / 0xF0 in every byte between them, immediately before and after each body.
    With arena (a high_arena.Arena) the layout goes to arena offset `base`, the arena's tensor is
    d_out and every out_off is base + the layout's: the phases then turn by base % 16; the layout,
    its guards and its low aliases are compared after the call"""
    nseg = len(segs)
    conns = conns or [T.TextConn(track=state is not None) for _ in range(nseg)]
    msg = np.zeros(nseg * mf, dtype=W.MSG_DTYPE)
    desc = np.zeros(nseg * mf, dtype=W.DESC_DTYPE)
    parts, pos, k = [], 0, 0
    for s, ms in enumerate(segs):
        assert len(ms) <= mf
        for i, (opcode, body, complete, continued, n_frames) in enumerate(ms):
            ph = phases[s][i] if phases else k % 16
            gap = 16 + (ph - (pos + 16)) % 16
            parts.append(np.resize(np.roll(np.array(POISON, np.uint8), k), gap))
            pos += gap
            parts.append(np.frombuffer(bytes(body), np.uint8))
            msg[s * mf + i] = (base + pos, len(body), i, n_frames, complete, continued)
            desc[s * mf + i]["type"] = 0 if continued else opcode
            desc[s * mf + i]["datalen"] = len(body)
            desc[s * mf + i]["ret"] = 2 + len(body)
            pos += len(body)
            k += 1
    parts.append(np.resize(np.array(POISON, np.uint8), 48))
    nmsg = torch.tensor([len(ms) for ms in segs], dtype=torch.int32, device=dev)
    d_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
    d_msg = torch.from_numpy(msg.view(np.uint8)).to(dev)
    if arena is not None:
        img = np.concatenate(parts)
        placed = arena.put(base, img)
        gv = validate(dev, arena.t, d_desc, d_msg, nmsg, mf, state, conns, segs, tag,
                      out_window=(base - 64, base + len(img) + 64))
        arena.check(placed, img, tag)
        return gv
    out = torch.from_numpy(np.concatenate(parts)).to(dev)
    assert out.data_ptr() % 16 == 0
    return validate(dev, out, d_desc, d_msg, nmsg, mf, state, conns, segs, tag)


def filler(n, seed=0):
    """n bytes of well-formed text: 1- to 4-byte sequences in turn, ASCII at the end"""
    unit = b"a" + SEQS[2] + b"bc" + SEQS[3] + b"d" + SEQS[4]
    b = (unit * (n // len(unit) + 2))[seed % len(unit):]
    while b[0] & 0xC0 == 0x80:                               # start on a sequence boundary
        b = b[1:]
    b = b[:n]
    k = T.tail_start(b)
    return b[:k] + b"x" * (n - k)


LENGTHS = [0, 1, 2, 3, 15, 16, 17] + [e + d for e in (CHUNK, ROW, TILE) for d in (-1, 0, 1)]


def lengths_and_phases(dev, **where):
    ms, ph = [], []
    for n in sorted(set(LENGTHS)):
        for p in range(16):
            for body in (b"a" * n, filler(n, p), (filler(n, p)[:-1] + b"\xe2") if n else b""):
                ms.append((1, body, 1, 0, 1))
                ms.append((1, body, 0, 0, 1) if p % 4 == 0 else (2, body, 1, 0, 1))
                ph += [p, p]
    half = len(ms) // 2
    gv = direct(dev, [ms[:half], ms[half:]], half + 3, phases=[ph[:half], ph[half:]], tag="lengths", **where)
    assert (gv == T.INVALID).any() and (gv == T.VALID).any() and (gv == T.NA).any()


def test_lengths_and_phases(dev):
    """every length around the chunk, row and tile sizes at every 16-B phase: ASCII, mixed
    sequences, and the same with the last byte cut to a lead"""
    lengths_and_phases(dev)


def sequences_across_every_edge(dev, **where):
    ms, ph = [], []
    for edge in (CHUNK, ROW, TILE, TILE + ROW, 2 * TILE):
        for p in range(16):
            for L, seq in SEQS.items():
                for j in range(1, L):
                    at = edge - p - j                        # j bytes of the sequence before the edge
                    if at < 0:
                        continue
                    body = bytearray(b"a" * (edge - p + 20))
                    body[at:at + L] = seq
                    ms.append((1, bytes(body), 1, 0, 1))
                    body[at + j] = 0x41 if p % 2 else 0xC2
                    ms.append((1, bytes(body), 1, 0, 1))
                    ph += [p, p]
    gv = direct(dev, [ms], len(ms), phases=[ph], tag="edges", **where)
    assert (gv[0, 0::2] == T.VALID).all() and (gv[0, 1::2] == T.INVALID).all()


def test_sequences_across_every_edge(dev):
    """a 2-, 3- and 4-byte sequence across every chunk, row and tile edge (every way of cutting
    it), at every phase; and the same with its byte after the edge broken"""
    sequences_across_every_edge(dev)


def test_single_bad_byte_positions(dev):
    """one bad byte first, last and on both sides of every row and tile edge of a multi-tile
    body; binary messages full of invalid bytes next to them stay NA"""
    n, p = 2 * TILE + ROW + 37, 7
    spots = {0, n - 1}
    for e in range(ROW, n + p, ROW):
        spots |= {e - p - 1, e - p}
    ms = [(1, filler(n, 3), 1, 0, 1)]
    for at in sorted(spots):
        b = bytearray(b"q" * n)
        b[at] = 0xFF if at % 2 else 0x80
        ms.append((1, bytes(b), 1, 0, 1))
        ms.append((2, b"\xff\xc0\x80" * 300, 1, 0, 1))
    gv = direct(dev, [ms], len(ms), phases=[[p] * len(ms)], tag="bad byte")
    assert gv[0, 0] == T.VALID and (gv[0, 1::2] == T.INVALID).all() and (gv[0, 2::2] == T.NA).all()


KOSME = bytes.fromhex("cebae1bdb9cf83cebcceb5")
AUTOBAHN = [
    bytes.fromhex("48656c6c6f2dc2b540c39fc3b6c3a4c3bcc3a0c3a12d5554462d382121"),          # 6.1 / 6.2
    KOSME + bytes.fromhex("eda080656469746564"),                                             # 6.3
    KOSME + bytes.fromhex("f4908080656469746564"),                                           # 6.4
    KOSME,                                                                                   # 6.5
] + [KOSME[:k] for k in range(1, 11)] + [                                                    # 6.6 truncations
    bytes.fromhex(h) for h in (
        "00", "c280", "e0a080", "f0908080", "f888808080", "fc8480808080",                    # 6.7, 6.8
        "7f", "dfbf", "efbfbf", "f48fbfbf", "f7bfbfbf", "fbbfbfbfbf", "fdbfbfbfbfbf",        # 6.9, 6.10
        "ed9fbf", "ee8080", "efbfbd", "f48fbfbf", "f4908080",                                # 6.11
        "80", "bf", "80bf", "80bf80", "80bf80bf", "80bf80bf80", "80bf80bf80bf",              # 6.12
        "c020c120c220c320df20", "e020e120ed20ef20", "f020f120f420f720", "f820f920fa20fb20", "fc20fd20",   # 6.13
        "c0", "e080", "f08080", "f8808080", "fc80808080", "df", "efbf", "f7bfbf", "fbbfbfbf", "fdbfbfbfbf",  # 6.14
        "c0e080f08080f8808080fc80808080dfefbff7bfbffbbfbfbffdbfbfbfbf",                      # 6.15
        "fe", "ff", "fefeffff",                                                              # 6.16
        "c0af", "e080af", "f08080af", "f8808080af", "fc80808080af",                          # 6.17
        "c1bf", "e09fbf", "f08fbfbf", "f887bfbfbf", "fc83bfbfbfbf",                          # 6.18
        "c080", "e08080", "f0808080", "f880808080", "fc8080808080",                          # 6.19
        "eda080", "edadbf", "edae80", "edafbf", "edb080", "edbe80", "edbfbf",                # 6.20
        "eda080edb080", "eda080edbfbf", "edadbfedb080", "edadbfedbfbf", "edae80edb080", "edafbfedbfbf",   # 6.21
        "efbfbe", "efbfbf", "f09fbfbe", "f09fbfbf", "f48fbfbe", "f48fbfbf",                  # 6.22
        "efbfbd", "f0908080", "e18080", "f1808080", "f3bfbfbf", "f4808080",                  # 6.23 and neighbours
        "e080", "ed", "eda0", "f0", "f08f", "f4", "f490", "f48f", "f48fbf", "e0a0",           # every truncation
    )] + [bytes(range(0x80, 0xC0))]                                                          # 6.12.8: all 64 continuations


def test_autobahn_section_6(dev):
    """Autobahn 6.x as byte literals: complete, open, after ASCII text, as a CLOSE reason, and
    cut in two batches at every byte"""
    ms = []
    for v in AUTOBAHN:
        ms += [(1, v, 1, 0, 1), (1, v, 0, 0, 1), (1, b"text " * 7 + v, 1, 0, 1), (8, b"\x03\xe8" + v, 1, 0, 1),
               (8, b"\xff\xff"[:len(v) % 3], 1, 0, 1), (8, b"\x03\xe8" + v, 1, 0, 2), (9, v, 1, 0, 1)]
    gv = direct(dev, [ms], len(ms), tag="autobahn")
    assert gv[0, 0] == T.VALID and gv[0, 7] == T.INVALID and gv[0, 3] == T.VALID and gv[0, 10] == T.INVALID
    assert gv[0, 5] == T.NA and gv[0, 6] == T.NA
    cuts = [(v, k) for v in AUTOBAHN for k in range(len(v) + 1) if len(v) <= 12]
    state = torch.zeros(len(cuts), dtype=torch.int32, device=dev)
    conns = [T.TextConn() for _ in cuts]
    direct(dev, [[(1, v[:k], 0, 0, 1)] for v, k in cuts], 1, conns, state, tag="autobahn cut a")
    direct(dev, [[(1, v[k:], 1, 1, 1)] for v, k in cuts], 1, conns, state, tag="autobahn cut b")
    assert not u32(state).any()


CARRY_SEQS = [bytes.fromhex(h) for h in ("c2a2", "e0a080", "e18080", "ed9fbf", "f0908080", "f1808080", "f48fbfbf",
                                         "e08080", "eda080", "f08f8080", "f4908080", "e0a041", "f09080c2")]


def carry_between_batches(dev, **where):
    cases = [(q, j) for q in CARRY_SEQS for j in range(1, len(q))]
    n = len(cases)
    state = torch.zeros(3 * n, dtype=torch.int32, device=dev)
    conns = [T.TextConn() for _ in range(3 * n)]
    # a: two batches; b: the bytes after the cut one per batch; c: an empty batch in between
    b1 = [[(1, b"ab" + q[:j], 0, 0, 1)] for q, j in cases] * 3
    direct(dev, b1, 2, conns, state, phases=[[13]] * (3 * n), tag="carry 1", **where)
    pend = u32(state)[:n] >> 24 & 3
    assert sorted(set(pend)) == [0, 1, 2, 3]               # FAILED ones have n = 0
    b2 = ([[(1, q[j:] + b"z", 1, 1, 1), (1, b"next", 1, 0, 1)] for q, j in cases] +
          [[(1, q[j:j + 1], 0, 1, 1)] for q, j in cases] + [[(1, b"", 0, 1, 1)] for q, j in cases])
    direct(dev, b2, 2, conns, state, phases=[[15, 0]] * (3 * n), tag="carry 2", **where)
    b3 = ([[] for _ in cases] + [[(1, q[j + 1:] + b"z", 1, 1, 3)] for q, j in cases] +
          [[(1, q[j:] + b"z", 0, 1, 1)] for q, j in cases])
    direct(dev, b3, 2, conns, state, phases=[[1]] * (3 * n), tag="carry 3", **where)
    assert not u32(state)[:2 * n].any() and (u32(state)[2 * n:] & T.ST_PENDING).all()


def test_carry_between_batches(dev):
    """sequences split between batches with 1, 2 and 3 pending bytes (every restricted lead, good
    and bad second bytes), one byte per batch, an empty continued body; all at two phases"""
    carry_between_batches(dev)


def test_state_rules(dev):
    """FAILED is sticky over two further batches; a continued non-text message stays NA; the
    state is unchanged for nmsg == 0 and for a batch of control messages only; a new message
    after the pending one closes; an open binary message clears the state"""
    state = torch.zeros(6, dtype=torch.int32, device=dev)
    conns = [T.TextConn() for _ in range(6)]
    bad = b"\xff\xc0" * 40
    direct(dev, [[(1, b"ok\xed\xa0", 0, 0, 1)], [(2, bad, 0, 0, 1)], [(1, b"x\xf0\x9f", 0, 0, 1)],
                 [(1, b"y\xe2\x82", 0, 0, 1)], [(1, b"z\xe2", 0, 0, 1)], [(1, b"fine", 1, 0, 1), (2, bad, 0, 0, 1)]],
           2, conns, state, tag="rules 1")
    s1 = u32(state).copy()
    assert s1[0] == T.ST_PENDING | T.ST_FAILED and s1[1] == 0 and s1[2] == T.ST_PENDING | 2 << 24 | 0x9FF0
    assert s1[5] == 0
    direct(dev, [[(1, b"plain ascii", 0, 1, 1)], [(2, bad, 0, 1, 1)], [],
                 [(9, b"\xff", 1, 0, 1), (10, b"", 1, 0, 1), (8, b"\x03\xe8\xff", 1, 0, 1)],
                 [(9, b"p", 1, 0, 1), (1, b"\x82\xac!", 1, 1, 2), (1, b"\xe2", 0, 0, 1)], [(2, b"", 1, 1, 1)]],
           3, conns, state, tag="rules 2")
    s2 = u32(state).copy()
    assert s2[0] == s1[0] and s2[2] == s1[2] and s2[3] == s1[3] and s2[4] == T.ST_PENDING | 1 << 24 | 0xE2
    gv = direct(dev, [[(1, b"more", 1, 1, 1), (1, b"new", 1, 0, 1)], [(2, bad, 1, 1, 1)], [(1, b"\x98\x80", 1, 1, 1)],
                      [(1, b"\xac", 1, 1, 1)], [(1, b"\x82\xac", 0, 1, 1)], []], 2, conns, state, tag="rules 3")
    assert list(gv[0, :2]) == [T.INVALID, T.VALID] and gv[1, 0] == T.NA and gv[2, 0] == T.VALID and gv[3, 0] == T.VALID
    assert not u32(state)[[0, 1, 2, 3, 5]].any() and u32(state)[4] == T.ST_PENDING


def test_without_state_every_batch_stands_alone(dev):
    gv = direct(dev, [[(1, b"\x82\xac", 1, 1, 1), (1, b"a\xe2", 0, 0, 1)], [(1, b"\xe2", 0, 1, 1)], []], 2, tag="no state")
    assert list(gv[0, :2]) == [T.NA, T.VALID] and gv[1, 0] == T.NA


# ------------------------------------------------------------------ behind the real reassembly

def text_frame(rng, b0, payload, masked=True):
    """reasm_cases.frame with a payload of our own"""
    f = bytearray(R.frame(rng, b0, len(payload), masked=masked))
    h = len(f) - len(payload)
    p = np.frombuffer(bytes(payload), np.uint8)
    if masked and len(p):
        p = p ^ np.resize(np.frombuffer(bytes(f[h - 4:h]), np.uint8), len(p))
    f[h:] = p.tobytes()
    return bytes(f)


def text_message(rng, payload, sizes, opcode=1, between=()):
    """a message in fragments of `sizes` (the last takes the rest); `between`: frames put after
    each fragment but the last"""
    cuts = [0] + [int(c) for c in np.cumsum(list(sizes)) if 0 < c < len(payload)] + [len(payload)]
    out = []
    for k in range(len(cuts) - 1):
        last = k == len(cuts) - 2
        out.append(text_frame(rng, (opcode if k == 0 else 0) | (0x80 if last else 0), payload[cuts[k]:cuts[k + 1]]))
        if not last:
            out += list(between)
    return out


def connection_frames(rng, way, s):
    """one connection's frames: text messages whose fragment sizes cut sequences, binary ones,
    and per way control frames between the fragments; some connections end with an open message"""
    frames = []
    for m in range(int(rng.integers(2, 5))):
        body = filler(int(rng.integers(0, 90)), int(rng.integers(0, 9)))
        if rng.random() < 0.3 and body:
            b = bytearray(body)
            b[int(rng.integers(0, len(b)))] = int(rng.choice([0x80, 0xC0, 0xED, 0xF4, 0xFF, 0xE0]))
            body = bytes(b)
        sizes = [int(x) for x in rng.integers(1, 9, int(rng.integers(0, 5)))]
        between = ()
        if way == "ctl":
            between = (text_frame(rng, 0x89, b"\xffping\xc0"),)
        elif way == "ex" and rng.random() < 0.5:
            between = (text_frame(rng, 0x09, b"" if rng.random() < 0.5 else b"\xe2\x82"),)   # joins the message
        frames += text_message(rng, body, sizes, opcode=1 if rng.random() < 0.8 else 2, between=between)
        if way == "ctl" and m == 1:
            frames.append(text_frame(rng, 0x88, b"\x03\xe8" + (b"bye \xe2\x82\xac" if s % 2 else b"bye \xe2\x82")))
    if s % 3 == 0:
        frames += text_message(rng, filler(40, s) + b"\xf0\x9f\x98\x80tail", [5, 9, 30])[:-1]   # no FIN: stays open
    return frames


def reassemble(way, b, flags, open_t):
    lib = _lib.load_text_lib()
    a = [W._ptr(b["d"]), b["d"].numel() - W.BATCH_PAD, W._ptr(b["so"]), W._ptr(b["sl"]), b["nseg"], b["mf"],
         W._ptr(b["desc"]), W._ptr(b["res"]), W._ptr(b["out"]), None, W._ptr(b["msg"]), W._ptr(b["nmsg"]), W._ptr(open_t)]
    st = W._stream(None)
    if way == "plain":
        rc = lib.websocketframeBatchReassembleDevice(*a, st)
    elif way == "ex":
        rc = lib.websocketframeBatchReassembleDeviceEx(*a, 0, None, st)
    else:
        rc = lib.websocketframeBatchReassembleDeviceCtl(*a, 0, None, flags, st)
    _lib.check(rc, "reassembly (%s)" % way, lib)


def wire_buffers(dev, segs_bytes, mf):
    so, sl, pos = [], [], 0
    for sb in segs_bytes:
        so.append(pos)
        sl.append(len(sb))
        pos += len(sb) + 3
    wire = np.zeros(pos + 1, np.uint8)
    for o, sb in zip(so, segs_bytes):
        wire[o:o + len(sb)] = np.frombuffer(sb, np.uint8)
    nseg = len(so)
    d = torch.zeros(len(wire) + 64, dtype=torch.uint8, device=dev)
    d[:len(wire)] = torch.from_numpy(wire).to(dev)
    b = dict(d=d, so=torch.tensor(so, dtype=torch.int64, device=dev), sl=torch.tensor(sl, dtype=torch.int64, device=dev),
             nseg=nseg, mf=mf, out=torch.full((len(wire) + 64,), 0xEE, dtype=torch.uint8, device=dev),
             desc=torch.zeros(nseg * mf * 32, dtype=torch.uint8, device=dev),
             msg=torch.zeros(nseg * mf * 32, dtype=torch.uint8, device=dev),
             res=torch.zeros(nseg * 16, dtype=torch.uint8, device=dev),
             nmsg=torch.zeros(nseg, dtype=torch.int32, device=dev))
    return wire, so, sl, b


def oracle_messages(way, wire, so, sl, mf, open_in):
    """the reassembly oracle's messages as the text oracle takes them"""
    if way == "ctl":
        od, _res, oms, oreg, oop, _ = oracle_reassemble_ctl(wire, so, sl, mf, open_in)
        imgs = [region_image(oreg[s], sl[s]) for s in range(len(so))]
    else:
        od, _res, oms, oreg, oop, _ = oracle_reassemble(wire, so, sl, mf, open_in)
        imgs = [oreg[s][1] for s in range(len(so))]
    segs = []
    for s in range(len(so)):
        ms = []
        for (o, n, first, nf, complete, cont) in oms[s]:
            ms.append((int(od[s * mf + first]["type"]), bytes(imgs[s][o - so[s]:o - so[s] + n]), complete, cont, nf))
        segs.append(ms)
    return segs, oms, oop


@pytest.mark.parametrize("way", ["plain", "ctl", "ex"])
@pytest.mark.parametrize("nseg,mf", [(1, 64), (3, 16), (3, 1), (1000, 16), (1000, 64)])
def test_through_the_reassembly(dev, way, nseg, mf):
    """every connection's frames in two batches (cut at a frame inside a message), d_open and the
    text state carried on the device; expected values from the reassembly oracle's messages"""
    rng = np.random.default_rng(1000 * nseg + mf)
    conns = [connection_frames(rng, way, s) for s in range(nseg)]
    cut = [int(rng.integers(1, len(f))) for f in conns]
    open_t = torch.zeros(nseg, dtype=torch.uint8, device=dev)
    state = torch.zeros(nseg, dtype=torch.int32, device=dev)
    tconns = [T.TextConn() for _ in range(nseg)]
    open_in = np.zeros(nseg, np.uint8)
    seen = set()
    for part in (0, 1):
        segs_bytes = [b"".join(f[:c] if part == 0 else f[c:]) for f, c in zip(conns, cut)]
        wire, so, sl, b = wire_buffers(dev, segs_bytes, mf)
        reassemble(way, b, W.REASM_CONTROL_DIRECT if way == "ctl" else 0, open_t)
        segs, oms, open_in = oracle_messages(way, wire, so, sl, mf, open_in)
        gv = validate(dev, b["out"], b["desc"], b["msg"], b["nmsg"], mf, state, tconns, segs, "%s part %d" % (way, part))
        gm, gn = b["msg"].cpu().numpy().view(W.MSG_DTYPE), b["nmsg"].cpu().numpy()
        for s in range(nseg):
            assert int(gn[s]) == len(oms[s])
            assert [tuple(int(x) for x in gm[s * mf + i]) for i in range(len(oms[s]))] == [tuple(m) for m in oms[s]]
        assert np.array_equal(open_t.cpu().numpy(), open_in)
        seen |= set(np.unique(gv[gv != SENTINEL]))
    if nseg >= 1000:
        assert seen == {T.NA, T.VALID, T.INVALID}


# ------------------------------------------------------------------ random text, one large message

def random_text(rng, n):
    """n bytes of random code points over all four lengths"""
    k = n // 2
    lo = np.array([0, 0x80, 0x800, 0x10000])[rng.integers(0, 4, k)]
    hi = np.array([0x80, 0x800, 0x10000, 0x110000])[np.searchsorted([0, 0x80, 0x800, 0x10000], lo)]
    cp = (lo + (rng.random(k) * (hi - lo)).astype(np.int64)).astype("<u4")
    cp[(cp >= 0xD800) & (cp < 0xE000)] = 0xFFFD
    b = cp.tobytes().decode("utf-32-le").encode("utf-8")[:n]
    k = T.tail_start(b)
    return b[:k] + b"." * (n - k)


def test_random_code_points(dev):
    """64 seeds of 1 MiB each, valid, and one corrupted copy of each (whatever the oracle says
    of the flip holds); every case asserted, alternately complete and open"""
    for base in range(0, 64, 16):
        segs = []
        for seed in range(base, base + 16):
            rng = np.random.default_rng(seed)
            good = random_text(rng, 1 << 20)
            bad = bytearray(good)
            bad[int(rng.integers(0, len(bad)))] = int(rng.integers(0, 256))
            segs += [[(1, good, 1, 0, 1)], [(1, bytes(bad), seed % 2, 0, 1)]]
        gv = direct(dev, segs, 1, state=torch.zeros(len(segs), dtype=torch.int32, device=dev), tag="random %d" % base)
        assert (gv[0::2, 0] == T.VALID).all() and (gv[1::2, 0] == T.INVALID).any()


def test_one_large_message(dev):
    """96 MiB in one message, its only error in the last byte: the work is split by bytes"""
    n, mf = 96 << 20, 1
    out = torch.full((n + 64,), 0x61, dtype=torch.uint8, device=dev)
    unit = torch.from_numpy(np.frombuffer("aé€😀bcdefghijkl".encode(), np.uint8).copy()).to(dev)
    assert unit.numel() == 21
    out[5:5 + (n // 21) * 21] = unit.repeat(n // 21)
    msg = np.zeros(1, dtype=W.MSG_DTYPE)
    desc = np.zeros(1, dtype=W.DESC_DTYPE)
    msg[0] = (5, n, 0, 1, 1, 0)
    desc[0]["type"] = 1
    d_msg, d_desc = torch.from_numpy(msg.view(np.uint8)).to(dev), torch.from_numpy(desc.view(np.uint8)).to(dev)
    nmsg = torch.ones(1, dtype=torch.int32, device=dev)
    verdict = torch.zeros(1, dtype=torch.int32, device=dev)
    fb = torch.zeros(1, dtype=torch.int32, device=dev)
    W.batch_validate_text_device(out, d_desc, d_msg, nmsg, mf, verdict, first_bad=fb)
    assert T.complete_ok(out[5:5 + n].cpu().numpy().tobytes())
    assert u32(verdict)[0] == T.VALID and u32(fb)[0] == T.NONE
    out[5 + n - 1] = 0xC3
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    W.batch_validate_text_device(out, d_desc, d_msg, nmsg, mf, verdict, first_bad=fb)
    ev[1].record()
    torch.cuda.synchronize()
    assert u32(verdict)[0] == T.INVALID and u32(fb)[0] == 0
    assert ev[0].elapsed_time(ev[1]) < 2000.0


def test_more_than_1024_plan_blocks(dev):
    """1021 segments of 257 slots: 262 397 slots in 1025 plan blocks, so every thread of the
    one-block scan of the block sums takes two. A segment lists 0 to 40 messages of a few bytes
    (the counts turn with a period of seven segments, the bodies with one of ten messages), and
    its slots move by one through the blocks from segment to segment: valid, invalid and
    unfinished text, binary messages, CLOSE reasons, the last message left open here and there."""
    bodies = [b"", b"a", SEQS[2], SEQS[3] + b"x", SEQS[4], b"\xc2", b"ab\xff", SEQS[3][:2], b"\xed\xa0\x80", "wörld".encode()]
    counts = [3, 0, 40, 1, 7, 18, 5]
    nseg, mf = 1021, 257
    assert (nseg * mf + 255) // 256 == 1025
    segs = []
    for s in range(nseg):
        ms = [(2 if (s + i) % 5 == 4 else 1, bodies[(3 * s + i) % len(bodies)], 1, 0, 1) for i in range(counts[s % 7])]
        if ms and s % 7 in (2, 4):
            ms[-1] = ms[-1][:2] + (0, 0, 1)                    # left open
        if s % 7 == 6:
            ms[1] = (8, b"\x03\xe8" + ms[1][1], 1, 0, 1)       # a CLOSE: its reason is checked
        segs.append(ms)
    gv = direct(dev, segs, mf, state=torch.zeros(nseg, dtype=torch.int32, device=dev), tag="1025 plan blocks")
    assert all((gv[:, :40] == v).any() for v in (T.VALID, T.INVALID, T.NA))


# ------------------------------------------------------------------ graph capture, workspace

def test_capture_and_workspace(dev):
    """reassembly + validation captured after one warm call and replayed on two different wires of
    the same framing; the workspace does not grow over 20 eager calls"""
    nseg, mf = 3, 16
    sizes = [[3, 5, 2, 70], [1, 1, 1], [4000, 7]]

    def wires(kind):
        out = []
        for s in range(nseg):
            body = filler(sum(sizes[s]) + 9, s + kind)
            if kind == 2 and s != 1:
                body = body[:3] + b"\xf5" + body[4:]
            out.append(b"".join(text_message(np.random.default_rng(5), body, sizes[s]) +
                                text_message(np.random.default_rng(6), b"\xe2\x82\xac" * 3, [4, 4])[:-1]))
        return out

    wire0, so, sl, b = wire_buffers(dev, wires(0), mf)
    open_t = torch.zeros(nseg, dtype=torch.uint8, device=dev)
    state = torch.zeros(nseg, dtype=torch.int32, device=dev)
    verdict = torch.full((nseg * mf,), SENTINEL, dtype=torch.int32, device=dev)
    fb = torch.zeros(nseg, dtype=torch.int32, device=dev)

    def call():
        reassemble("ctl", b, W.REASM_CONTROL_DIRECT, open_t)
        W.batch_validate_text_device(b["out"], b["desc"], b["msg"], b["nmsg"], mf, verdict, text_state=state, first_bad=fb)

    stat = C.c_ulonglong(0)
    lib = _lib.load_text_lib()
    call()
    torch.cuda.synchronize()
    assert lib.websocketframeGpuGetStat(b"workspace_bytes", C.byref(stat)) == 0
    held = stat.value
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    assert lib.websocketframeGpuGetStat(b"workspace_bytes", C.byref(stat)) == 0
    assert stat.value == held and held > 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for kind in (1, 2):
        wire = np.zeros(len(wire0), np.uint8)
        for o, sb in zip(so, wires(kind)):
            wire[o:o + len(sb)] = np.frombuffer(sb, np.uint8)
        b["d"][:len(wire)] = torch.from_numpy(wire).to(dev)
        open_t.zero_()
        state.zero_()
        verdict.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        segs, _oms, _oop = oracle_messages("ctl", wire, so, sl, mf, np.zeros(nseg, np.uint8))
        gv, gs, gf = u32(verdict).reshape(nseg, mf), u32(state), u32(fb)
        for s in range(nseg):
            ov, ofb, oword = T.TextConn().batch(segs[s])
            assert list(gv[s, :len(ov)]) == ov and (gv[s, len(ov):] == SENTINEL).all(), (kind, s)
            assert int(gf[s]) == ofb and int(gs[s]) == oword, (kind, s)
        assert (gv == T.INVALID).any() == (kind == 2)
    del g
