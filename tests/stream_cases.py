"""Directed raw-stream cases for the chunk-parallel walk (util_amd/csrc/ws_stream.hip), small enough
that every chunk edge lies at an address the test computes: a base stream of about 1.25 MiB of masked
client frames with 20-90 B payloads (mean wire frame <= 64 B: chunks of 64 KiB, windows of 8 KiB by
tests/rwplan_model.py) and *splices* of it — the bytes of whole frames between two frame starts after
the sample replaced by another framing of the same total length, filler frames absorbing the
remainder — so the sample, the length and with them the geometry stay what the model says. Each
builder returns Case(name, wire, max_frames, cells, opts): `cells` are the claims the case makes
("chunk 7: header of form 126 cut after byte 3 by the chunk start"), each checked against the oracle's
frame offsets under the model's geometry by tests/test_stream_cases.py (no GPU) and again under the
geometry read back from the device by tests/test_gpu_stream_edges.py."""
import ctypes
import os
import subprocess
import tempfile
from collections import namedtuple

import numpy as np

import rwplan_model as M
from oracle_lib import oracle_segments

BASE_BYTES = 1310720                       # 1.25 MiB: 20 chunks of 64 KiB less the sample's 4
BIG_MF = 1 << 16
DEFAULT_OPTS = dict(stream_split=8, stream_split2=48, stream_c0=3, stream_c1=2)

Case = namedtuple("Case", "name wire max_frames cells opts")
Case.__new__.__defaults__ = (None,)


# ---- frames

def frame(rng, plen, masked=True, b0=0x82, body=None):
    """one frame's wire bytes; body: payload bytes as they lie on the wire (default random)"""
    m = 0x80 if masked else 0
    if plen < 126:
        h = bytes([b0, m | plen])
    elif plen <= 0xFFFF:
        h = bytes([b0, m | 126]) + plen.to_bytes(2, "big")
    else:
        h = bytes([b0, m | 127]) + plen.to_bytes(8, "big")
    if masked:
        h += rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
    if body is None:
        body = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
    assert len(body) == plen
    return h + body


def hdr_len(form, masked):
    return {125: 2, 126: 4, 127: 10}[form] + (4 if masked else 0)


FORM_PLEN = {125: 50, 126: 300, 127: 70000}     # a payload of each header form


def filler(rng, n):
    """masked frames of 20-90 B payloads (the last one whatever is left, 0-125 B) of exactly n bytes;
    a zero-length masked frame is 6 B, so every n of 0 or >= 6 can be framed"""
    assert n == 0 or n >= 6, n
    out = []
    while n > 131:
        f = 6 + int(rng.integers(20, 91))
        out.append(frame(rng, f - 6))
        n -= f
    if n:
        out.append(frame(rng, n - 6))
    return b"".join(out)


def frame_offsets(wire, max_frames=BIG_MF):
    """(frame offsets, wire lengths, result) of the oracle's loop over the whole stream"""
    od, orr = oracle_segments(wire.copy(), [0], [len(wire)], max_frames)
    n = int(orr[0]["n_frames"])
    return od["frame_off"][:n].astype(np.int64), od["ret"][:n].astype(np.int64), orr[0]


_base = {}


def base_stream():
    """(wire, frame offsets, frame lengths): lengths change nearly every frame, so a chunk walk's
    sample keeps the walk hint set"""
    if not _base:
        rng = np.random.default_rng(9001)
        parts, total = [], 0
        while total < BASE_BYTES - 300:
            f = frame(rng, int(rng.integers(20, 91)), b0=int(rng.choice([0x01, 0x02, 0x81, 0x82, 0x80, 0x00])))
            parts.append(f)
            total += len(f)
        parts.append(filler(rng, BASE_BYTES - total))
        wire = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        fo, fl, res = frame_offsets(wire)
        assert int(res["consumed"]) == BASE_BYTES == len(wire)
        _base["v"] = (wire, fo, fl)
    return _base["v"]


# ---- geometry of a case under the model

def sample_of(fo, fl, length):
    """(P1, frames before it, mean, the sample's longest frame) for a walk that starts at 0; P1 None:
    the walk ends in the sample"""
    send = M.SAMPLE if length > M.SAMPLE else length
    k = int(np.searchsorted(fo, send))
    if k >= len(fo):
        return None, len(fo), 0, 0
    P1 = int(fo[k])
    return P1, k, M.mean_of(0, P1, k), int(fl[:k].max()) if k else 0


def geometry(wire, seen=0, lead=0, opts=None, fo=None, fl=None):
    """the model's plan of a skip-path call on this stream after a walk whose longest frame was `seen`;
    None when the walk never reaches the chunks"""
    if fo is None:
        fo, fl, _ = frame_offsets(wire)
    o = dict(DEFAULT_OPTS, **(opts or {}))
    P1, nf, mean, smax = sample_of(fo, fl, len(wire))
    if P1 is None or len(wire) < M.MIN_STREAM or M.short_rest(P1, len(wire), mean):
        return None
    g = M.call_plan(P1, len(wire), mean, max(smax, seen), lead, o["stream_split"], o["stream_split2"], o["stream_c0"],
                    o["stream_c1"])
    return g, P1, nf


def chunks_of(g):
    """[(part, local index, cs, cend, H)] of every chunk, in stream order"""
    out = []
    for k in range(g.nparts):
        t = g.parts[k]
        for c in range(t.n):
            out.append((k, c, t.P + c * t.C, t.P + (c + 1) * t.C, t.H))
    return out


def base_chunks():
    """the base stream's chunk starts under the default options: one part of 64 KiB chunks"""
    wire, fo, fl = base_stream()
    g, P1, nf = geometry(wire, fo=fo, fl=fl)
    ch = chunks_of(g)
    assert all(t.n == 0 for t in g.parts[:g.nparts - 1]) and g.parts[g.nparts - 1].C == 65536
    assert g.parts[g.nparts - 1].H == 8192 and len(ch) == M.ceil_div(BASE_BYTES - P1, 65536)
    return g, P1, ch


# ---- the splice

def splice(wire, fo, items, rng):
    """items: [(absolute position, bytes)] in order, not touching; each lands at its position, filler
    frames from the last base frame start at least 6 B before it and up to the first base frame start
    at least 6 B after it. Length and every byte before the first filler unchanged."""
    w = wire.copy()
    P1 = int(fo[np.searchsorted(fo, M.SAMPLE)])
    prev_b = P1
    for pos, data in items:
        i = int(np.searchsorted(fo, pos))
        a = pos if i < len(fo) and int(fo[i]) == pos else int(fo[np.searchsorted(fo, pos - 6, side="right") - 1])
        end = pos + len(data)
        j = int(np.searchsorted(fo, end))
        if j < len(fo) and int(fo[j]) == end:
            b = end
        else:
            j = int(np.searchsorted(fo, end + 6))
            b = int(fo[j]) if j < len(fo) else len(wire)
        assert b == end or b - end >= 6, "no room for a filler after the item"
        assert a >= prev_b and a >= P1, (a, prev_b, P1)
        seq = filler(rng, pos - a) + data + filler(rng, b - end)
        assert len(seq) == b - a
        w[a:b] = np.frombuffer(seq, dtype=np.uint8)
        prev_b = b
    return w


# ---- the fill of the walk's per-chunk pools, by the scalar chunk-walk model (tests/c/link_host.cpp)

POOL_CAPS = {"wcap": 256, "s0": 40, "d": 4}       # RW_WCAP, RW_S0, RW_D (capc: the part's own)
_pool_lib = []


def pool_counts(wire, g, lead=0):
    """{global chunk: (most plausible positions in one 4 KiB wave span, survivors of two headers, window walks
    that leave the window, their distinct exits)} under geometry g at buffer phase `lead`"""
    if not _pool_lib:
        d = tempfile.mkdtemp(prefix="link_host")
        so = os.path.join(d, "liblink_host.so")
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "link_host.cpp")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", src, "-o", so], check=True)
        lib = ctypes.CDLL(so)
        lib.ws_link_host_pool_counts.restype = ctypes.c_longlong
        lib.ws_link_host_pool_counts.argtypes = [ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_ulonglong,
                                                 ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint,
                                                 ctypes.c_void_p, ctypes.c_ulonglong]
        _pool_lib.append(lib)
    buf = np.concatenate([wire, np.zeros(64, dtype=np.uint8)])
    out, at = {}, 0
    for k in range(g.nparts):
        t = g.parts[k]
        if not t.n:
            continue
        end = g.parts[k + 1].P if k + 1 < g.nparts else len(wire)
        cnt = np.zeros(4 * t.n, dtype=np.uint32)
        n = _pool_lib[0].ws_link_host_pool_counts(buf.ctypes.data, len(buf), end, t.P, t.C, t.H, lead,
                                                  1 if int(wire[t.P + 1]) & 0x80 else 0, cnt.ctypes.data, t.n)
        assert n == t.n, (n, t)
        for c in range(t.n):
            out[at + c] = tuple(int(x) for x in cnt[4 * c:4 * c + 4])
        at += t.n
    return out


# ---- cells: a claim about one chunk, checked on frame offsets under a geometry

def check_cell(cell, wire, max_frames, g, fo, fl, res, lead=0):
    """raises AssertionError unless the claim holds"""
    ch = chunks_of(g)
    kind = cell[0]
    if kind == "pool":                                   # chunk c fills that pool below (at or under) / above its cap
        _, c, which, side = cell
        n = pool_counts(wire, g, lead)[c]["wcap capc s0 d".split().index(which)]
        cap = g.parts[ch[c][0]].capc if which == "capc" else POOL_CAPS[which]
        assert (0 < n <= cap if which == "d" else 0 < n < cap) if side == "below" else n > cap, (cell, n, cap)
        return
    starts = set(int(x) for x in fo)
    if kind == "start":                                  # a frame starts at cs + d
        _, c, d = cell
        assert ch[c][2] + d in starts, cell
    elif kind == "hdr_cut":                              # the header of that form is cut by cs after byte k
        _, c, form, masked, k = cell
        p = ch[c][2] - k
        # (an incomplete last frame has no descriptor: the walk stops at it)
        assert (p in starts or int(res["consumed"]) == p) and 1 <= k < hdr_len(form, masked), cell
        b1 = int(wire[p + 1])
        assert (b1 & 0x7F if (b1 & 0x7F) >= 126 else 125) == form and bool(b1 & 0x80) == masked, cell
    elif kind == "zero_end":                             # a zero-length frame ends exactly at cs
        _, c = cell
        i = int(np.searchsorted(fo, ch[c][2])) - 1
        assert int(fo[i]) + 6 == ch[c][2] and int(fl[i]) == 6 and ch[c][2] in starts, cell
    elif kind == "entry":                                # the chain's first frame start in the chunk is cs + d
        _, c, d = cell
        i = int(np.searchsorted(fo, ch[c][2]))
        assert int(fo[i]) == ch[c][2] + d, (cell, int(fo[i]) - ch[c][2])
        assert (d < ch[c][4]) == (cell[2] < ch[c][4])
    elif kind == "long":                                 # a frame of n wire bytes starts in chunk c, in its window's last position if asked
        _, c, n, at_window_end = cell
        i = int(np.searchsorted(fo, ch[c][2]))
        js = [j for j in range(i, min(i + 400, len(fo))) if int(fl[j]) == n and int(fo[j]) < ch[c][3]]
        assert js, cell
        if at_window_end:
            assert int(fo[js[0]]) == ch[c][2] + ch[c][4] - 1, cell
    elif kind == "next_hdr":                             # a frame starts in chunk c's window and the header after it lies at cend + d
        _, c, d = cell
        js = [j for j in range(len(fo)) if ch[c][2] <= int(fo[j]) < ch[c][2] + ch[c][4] and int(fo[j]) + int(fl[j]) == ch[c][3] + d]
        assert js and c + 1 < len(ch), cell
    elif kind == "r2_jump":                              # a wrong start 10 B before the window's end: its frame jumps past the
        _, c = cell                                      # end onto a plausible header, the header after that is not one
        p = ch[c][2] + ch[c][4] - 10
        ok = lambda q: not int(wire[q]) & 0x70 and (int(wire[q]) & 15) in (0, 1, 2, 8, 9, 10) and int(wire[q + 1]) & 0x80
        assert p not in starts and ok(p) and int(wire[p + 1]) & 0x7F < 126, cell
        q = p + 6 + (int(wire[p + 1]) & 0x7F)
        assert q >= ch[c][2] + ch[c][4] and q not in starts and ok(q) and int(wire[q + 1]) & 0x7F < 126, cell
        r = q + 6 + (int(wire[q + 1]) & 0x7F)
        assert r < ch[c][3] and not ok(r), cell
    elif kind == "last_frame_long":
        assert int(fl[-1]) >= cell[1] and int(fo[-1]) + int(fl[-1]) == len(wire), cell
    elif kind == "len_at":                               # the stream ends d bytes into its last chunk
        _, d = cell
        cs = ch[-1][2]
        assert len(wire) - cs == (d if d else ch[-1][3] - ch[-1][2]), (cell, len(wire) - cs)
    elif kind == "trunc":                                # the last frame is incomplete: k bytes of it are there
        _, k = cell
        assert int(res["status"]) == 0 and len(wire) - int(res["consumed"]) == k, (cell, res)
    elif kind == "max_at":                               # max_frames = frames before `what` + d
        _, what, d, want = cell
        if what.startswith("handoff"):                   # want: the frames before the chain's entry into that part
            k = int(what[-1])
            assert g.nparts > k and g.parts[k].n and want == int(np.searchsorted(fo, g.parts[k].P)), cell
        assert max_frames == want + d, cell
        assert int(res["n_frames"]) == min(max_frames, len(fo)), cell
    elif kind == "end":                                  # a bad header at the chunk's first / last chain frame
        _, c, where, what = cell[:4]
        p = cell[4]                                     # the chain reaches the bad header at p, in chunk c
        stop = int(res["consumed"])
        assert p in starts or stop == p, (cell, res)
        assert ch[c][2] <= p < ch[c][3], (cell, p)
        if what == "wrap":                               # a 64-bit length past the stream: the walk stops there
            assert stop == p, (cell, res)
        elif what == "unmasked":                         # a frame of the chain the speculation of a masked stream refuses
            assert p in starts and not int(wire[p + 1]) & 0x80, cell
        else:                                            # ... and one with RSV bits (the oracle takes them, and any opcode)
            assert int(wire[p]) & 0x70, cell
        if where.startswith("part"):                     # ... the chain's entry into that part
            k = int(where[-1])
            assert g.nparts > k and ch[c][0] == k and ch[c][1] == 0 and g.parts[k].n, cell
        if where == "first" or where.startswith("part"):  # no frame of the chain starts in the chunk before it
            assert not [x for x in starts if ch[c][2] <= x < p], (cell, p)
        else:                                            # in the chunk's (the stream's) last 300 bytes
            assert p >= min(ch[c][3], len(wire)) - 300, (cell, p)
    elif kind == "split":                                # the parts' shape
        what = cell[1]
        n = [g.parts[k].n for k in range(g.nparts)]
        if what == "part0_empty":
            assert g.nparts >= 2 and n[0] == 0, cell
        elif what == "middle_empty":
            assert g.nparts == 3 and n[1] == 0 and n[0] > 0, (cell, n)
        elif what == "cut_on_chunk_start":
            assert g.nparts >= 2 and n[0] > 0 and cell[2] == g.parts[1].P, (cell, g)
        elif what == "cut_one_byte_inside":
            assert g.nparts >= 2 and n[0] >= 1 and (cell[2] - g.parts[0].P) % g.parts[0].C == 1, (cell, g)
            assert g.parts[1].P - cell[2] == g.parts[0].C - 1, (cell, g)
        elif what == "two_parts":
            assert g.nparts == 2, cell
        elif what == "three_live_parts":
            assert g.nparts == 3 and all(n), (cell, n)
        else:
            raise AssertionError(cell)
    else:
        raise AssertionError("unknown cell %r" % (cell,))


CELL_KINDS = (["start -1", "start 0", "start 1", "zero_end", "entry H-1", "entry H", "long C-H", "long C", "long C+1",
               "long 3C", "long at window end", "last_frame_long"] +
              ["hdr_cut %d %d %d" % (f, m, k) for f in (125, 126, 127) for m in (1, 0) for k in range(1, hdr_len(f, bool(m)))] +
              ["len_at %s" % d for d in ("0", "1", "2", "H-1", "H", "H+1")] +
              ["trunc %s" % k for k in ("1", "2", "3", "4", "5", "payload-1")] +
              ["max_at %s %+d" % (w, d) for w in ("entry", "sample", "total") for d in (-1, 0, 1)] +
              ["end %s %s" % (w, k) for w in ("first", "last") for k in ("garbage", "wrap", "unmasked", "rsv")] +
              ["split %s" % s for s in ("part0_empty", "middle_empty", "cut_on_chunk_start", "cut_one_byte_inside", "two_parts",
                                        "three_live_parts")] +
              ["next_hdr %+d" % d for d in (-1, 0, 1)] + ["r2_jump"] +
              ["pool %s %s" % (w, sd) for w in ("wcap", "capc", "s0", "d") for sd in ("below", "above")] +
              ["max_at handoff%d %+d" % (k, d) for k in (1, 2) for d in (-1, 0, 1)] +
              ["end part%d %s" % (k, w) for k in (1, 2) for w in ("garbage", "wrap", "unmasked", "rsv")])


def cell_kind(cell, g):
    """the CELL_KINDS name a cell counts for"""
    k = cell[0]
    H = g.parts[g.nparts - 1].H
    C = g.parts[g.nparts - 1].C
    if k == "start":
        return "start %d" % cell[2]
    if k == "hdr_cut":
        return "hdr_cut %d %d %d" % (cell[2], int(cell[3]), cell[4])
    if k == "entry":
        return "entry H-1" if cell[2] == H - 1 else "entry H"
    if k == "long":
        return "long at window end" if cell[3] else "long %s" % {C - H: "C-H", C: "C", C + 1: "C+1", 3 * C: "3C"}[cell[2]]
    if k == "next_hdr":
        return "next_hdr %+d" % cell[2]
    if k == "pool":
        return "pool %s %s" % (cell[2], cell[3])
    if k == "len_at":
        return "len_at %s" % {0: "0", 1: "1", 2: "2", H - 1: "H-1", H: "H", H + 1: "H+1"}[cell[1]]
    if k == "trunc":
        return "trunc %s" % (cell[1] if cell[1] <= 5 else "payload-1")
    if k == "max_at":
        return "max_at %s %+d" % (cell[1], cell[2])
    if k == "end":
        return "end %s %s" % (cell[2], cell[3])
    if k == "split":
        return "split %s" % cell[1]
    return k


# ---- builders (every group places its items at two chunk indices: a middle chunk and the last)

def _long_frame(rng, n):
    """a masked frame of exactly n wire bytes (n >= 6)"""
    for h in (6, 8, 14):
        p = n - h
        if p >= 0 and hdr_len(125 if p < 126 else 126 if p <= 0xFFFF else 127, True) == h:
            return frame(rng, p)
    raise AssertionError(n)


def chunk_start_cases():
    wire, fo, fl = base_stream()
    g, P1, ch = base_chunks()
    rng = np.random.default_rng(9100)
    last = len(ch) - 1
    out = []
    for d in (-1, 0, 1):
        items = [(ch[c][2] + d, frame(rng, 40)) for c in (3, last)]
        out.append(Case("start%+d" % d, splice(wire, fo, items, rng), BIG_MF, [("start", c, d) for c in (3, last)]))
    items = [(ch[c][2] - 6, frame(rng, 0) + frame(rng, 33)) for c in (5, last)]
    out.append(Case("zero_end", splice(wire, fo, items, rng), BIG_MF, [("zero_end", c) for c in (5, last)]))
    # header cuts: the short forms many to a wire (one chunk start each), the 64-bit form (a frame longer
    # than a chunk) at a middle chunk and at the last one in turn
    for form in (125, 126):
        for masked in (True, False):
            cuts = list(range(1, hdr_len(form, masked)))
            pairs = list(zip(range(2, 2 + len(cuts)), cuts))
            items = [(ch[c][2] - k, frame(rng, FORM_PLEN[form], masked)) for c, k in pairs]
            out.append(Case("hdr_cut_%d_%d_mid" % (form, masked), splice(wire, fo, items, rng), BIG_MF,
                            [("hdr_cut", c, form, masked, k) for c, k in pairs]))
            for k in cuts:                                   # and each at the last chunk's start
                out.append(Case("hdr_cut_%d_%d_%d_last" % (form, masked, k),
                                splice(wire, fo, [(ch[last][2] - k, frame(rng, FORM_PLEN[form], masked))], rng), BIG_MF,
                                [("hdr_cut", last, form, masked, k)]))
    for masked in (True, False):
        for k in range(1, hdr_len(127, masked)):
            for c in (4 + k % 3, last):
                room = len(wire) - (ch[c][2] - k)
                plen = FORM_PLEN[127] if room > FORM_PLEN[127] + 100 else 65536 + (room - 65536 - hdr_len(127, masked) - 40) % 7
                # the last chunk is shorter than a 64 KiB payload when the stream ends early in it: the frame
                # is then the stream's incomplete last frame, its header still cut by the chunk start
                if room < 65536 + 60:
                    w2 = wire.copy()
                    a = int(fo[np.searchsorted(fo, ch[c][2] - k - 6, side="right") - 1])
                    seq = filler(rng, ch[c][2] - k - a) + frame(rng, 70000, masked)
                    w2[a:] = np.frombuffer(seq[:len(wire) - a], dtype=np.uint8)
                    out.append(Case("hdr_cut_127_%d_%d_last" % (masked, k), w2, BIG_MF, [("hdr_cut", c, 127, masked, k)]))
                else:
                    items = [(ch[c][2] - k, frame(rng, plen, masked))]
                    out.append(Case("hdr_cut_127_%d_%d_c%d" % (masked, k, c), splice(wire, fo, items, rng), BIG_MF,
                                    [("hdr_cut", c, 127, masked, k)]))
    return out


def window_and_long_cases():
    wire, fo, fl = base_stream()
    g, P1, ch = base_chunks()
    rng = np.random.default_rng(9200)
    C, H = 65536, 8192
    last = len(ch) - 1
    out = []
    # the chain's first frame start in the chunk at cs + H - 1 (the window's last position) and at cs + H
    # (no entry in the window: the chunk is walked): a frame that starts 40 B before cs and ends there
    for d in (H - 1, H):
        items = [(ch[c][2] - 40, _long_frame(rng, 40 + d) + frame(rng, 25)) for c in (6, last)]
        out.append(Case("entry_%d" % d, splice(wire, fo, items, rng), BIG_MF, [("entry", c, d) for c in (6, last)]))
    for n in (C - H, C, C + 1, 3 * C):
        cs_list = (2, last - 4) if n == 3 * C else (2, last - 2)
        items = [(ch[c][2] + 100, _long_frame(rng, n)) for c in cs_list]
        out.append(Case("long_%d" % n, splice(wire, fo, items, rng), BIG_MF, [("long", c, n, False) for c in cs_list]))
    # one starting in the window's last position and covering the next chunk: a middle chunk, and the last
    # chunk that has a next one
    items = [(ch[c][2] + H - 1, _long_frame(rng, C + C // 2)) for c in (3, last - 1)]
    out.append(Case("long_from_window_end", splice(wire, fo, items, rng), BIG_MF,
                    [("long", c, C + C // 2, True) for c in (3, last - 1)]))
    # a candidate in the window whose next header lies at cend - 1, cend, cend + 1 (R1 steps on only while pos < cend)
    for d in (-1, 0, 1):
        items = [(ch[c][2] + 100, _long_frame(rng, C - 100 + d) + frame(rng, 31)) for c in (4, last - 1)]
        out.append(Case("next_hdr%+d" % d, splice(wire, fo, items, rng), BIG_MF, [("next_hdr", c, d) for c in (4, last - 1)]))
    # a wrong start 10 B before the window's end inside a true frame's payload: a plausible header whose frame
    # jumps past the window onto another plausible header, then 0xFF (R2's extra headers refuse it)
    body = bytearray(rng.integers(0, 256, 600, dtype=np.uint8).tobytes())
    body[100:106] = bytes([0x82, 0x80 | 100, 1, 2, 3, 4])
    body[206:212] = bytes([0x81, 0x80 | 50, 5, 6, 7, 8])
    body[262:264] = b"\xff\xff"
    items = [(ch[c][2] + H - 10 - 100 - 8, frame(rng, 600, body=bytes(body))) for c in (5, last)]
    out.append(Case("r2_jump", splice(wire, fo, items, rng), BIG_MF, [("r2_jump", c) for c in (5, last)]))
    # one that is the stream's last frame
    a = int(fo[np.searchsorted(fo, len(wire) - (C + 5000))])
    w2 = wire.copy()
    w2[a:] = np.frombuffer(_long_frame(rng, len(wire) - a), dtype=np.uint8)
    out.append(Case("last_frame_long", w2, BIG_MF, [("last_frame_long", C)]))
    return out


def stream_end_cases():
    """the stream cut (a shorter length: its own geometry by the model, the same sample)"""
    wire, fo, fl = base_stream()
    g, P1, ch = base_chunks()
    H = 8192
    out = []
    for c in (len(ch) - 1, len(ch) - 6):
        for d in (0, 1, 2, H - 1, H, H + 1):
            n = ch[c][2] + d if d else ch[c][2]            # d 0: chunk c - 1 is the last, exactly full
            out.append(Case("len_c%d_%d" % (c, d), wire[:n].copy(), BIG_MF, [("len_at", d)]))
    # the last frame truncated after each header byte and one byte short of its payload
    i = len(fo) - 40
    for k in (1, 2, 3, 4, 5, int(fl[i]) - 1):
        out.append(Case("trunc_%d" % k, wire[:int(fo[i]) + k].copy(), BIG_MF, [("trunc", k)]))
    return out


def count_cases():
    wire, fo, fl = base_stream()
    g, P1, ch = base_chunks()
    nsample = int(np.searchsorted(fo, P1))
    out = []
    for what, want in (("entry", int(np.searchsorted(fo, ch[7][2]))), ("entry", int(np.searchsorted(fo, ch[-1][2]))),
                       ("sample", nsample), ("total", len(fo))):
        for d in (-1, 0, 1):
            out.append(Case("max_%s_%d%+d" % (what, want, d), wire, want + d, [("max_at", what, d, want)]))
    return out


def ending_cases():
    wire, fo, fl = base_stream()
    g, P1, ch = base_chunks()
    rng = np.random.default_rng(9300)
    bad = {"garbage": bytes([0x37, 0x91, 0xC3, 0x5A, 0x77, 0x13, 0xFE, 0x09, 0x44, 0xB2, 0x61, 0x0F, 0xA8, 0x3C]),
           "wrap": bytes([0x82, 0xFF]) + (0xFFFFFFFFFFFFFFF0).to_bytes(8, "big") + bytes(4),
           "unmasked": frame(rng, 30, masked=False), "rsv": frame(rng, 30, b0=0xC2)}
    out = []
    for what, data in bad.items():
        for c in (4, len(ch) - 1):
            i = int(np.searchsorted(fo, ch[c][2]))               # the chunk's first frame
            w2 = wire.copy()
            w2[int(fo[i]):int(fo[i]) + len(data)] = np.frombuffer(data, dtype=np.uint8)
            out.append(Case("end_first_%s_c%d" % (what, c), w2, BIG_MF, [("end", c, "first", what, int(fo[i]))]))
            j = int(np.searchsorted(fo, min(ch[c][3], len(wire)) - 150)) if c < len(ch) - 1 else len(fo) - 3
            j = min(j, int(np.searchsorted(fo, min(ch[c][3], len(wire)))) - 1)   # a frame that starts in the chunk's last bytes
            if int(fo[j]) + len(data) <= len(wire):
                w3 = wire.copy()
                w3[int(fo[j]):int(fo[j]) + len(data)] = np.frombuffer(data, dtype=np.uint8)
                out.append(Case("end_last_%s_c%d" % (what, c), w3, BIG_MF, [("end", c, "last", what, int(fo[j]))]))
    return out


def split_cases():
    """the base stream under split options the model says give each shape (lead 0)"""
    wire, fo, fl = base_stream()
    _, P1, _ = base_chunks()
    n = len(wire)
    npieces = (n - 1) // M.PIECE + 1
    out = [Case("split_defaults", wire, BIG_MF, [("split", "part0_empty")], dict(DEFAULT_OPTS))]
    # the cut on a chunk start of part 0's grid / one byte inside a chunk: cuts are whole pieces, so look for
    # the piece whose first byte has that relation to P1's grid (chunks of 64 KiB: c0 = 0)
    for what, rel in (("cut_on_chunk_start", 0), ("cut_one_byte_inside", 1)):
        found = None
        for s in range(1, 256):
            x = max(1, npieces * s // 256) * M.PIECE
            if x > P1 and (x - P1) % 65536 == rel:
                found = (s, x)
                break
        if found:
            out.append(Case("split_" + what, wire, BIG_MF, [("split", what, found[1])],
                            dict(stream_split=found[0], stream_split2=0, stream_c0=0, stream_c1=0)))
    out.append(Case("split_middle_empty", wire, BIG_MF, [("split", "middle_empty")],
                    dict(stream_split=100, stream_split2=103, stream_c0=0, stream_c1=6)))
    out.append(Case("split2_le_split", wire, BIG_MF, [("split", "two_parts")],
                    dict(stream_split=128, stream_split2=64, stream_c0=6, stream_c1=0)))
    out.append(Case("split_three_parts_c6", wire, BIG_MF, [("split", "three_live_parts")],
                    dict(stream_split=80, stream_split2=160, stream_c0=6, stream_c1=6)))
    out.append(Case("split_three_parts_c0", wire, BIG_MF, [("split", "three_live_parts")],
                    dict(stream_split=80, stream_split2=160, stream_c0=0, stream_c1=0)))
    return out


def pool_cases():
    """both sides of each per-chunk pool at the base geometry (capc 256), at a middle chunk and the last:
    the base stream itself (about 134 frame starts of 26-96 B in a window: under RW_WCAP and capc, one
    exit, over RW_S0); a window of frames of 400 B payloads (about 20 starts: under RW_S0); a window of
    true zero-length frames (1365 starts: over RW_WCAP, capc and RW_S0, one exit); and a window inside
    one long frame whose payload holds six interleaved chains of plausible 96-byte frames that never
    merge (six distinct exits: over RW_D, and over the other three)"""
    wire, fo, fl = base_stream()
    g, P1, ch = base_chunks()
    rng = np.random.default_rng(9950)
    last = len(ch) - 1
    H = 8192
    two = (7, last)
    out = [Case("pool_base", wire, BIG_MF, [("pool", c, w, sd) for c in two
                                            for w, sd in (("wcap", "below"), ("capc", "below"), ("s0", "above"), ("d", "below"))])]
    sparse = b"".join(frame(rng, 400) for _ in range(24))                     # from just before cs to past the window
    items = [(ch[c][2] - 100, sparse) for c in two]
    out.append(Case("pool_sparse", splice(wire, fo, items, rng), BIG_MF, [("pool", c, "s0", "below") for c in two]))
    zeros = b"".join(frame(rng, 0, body=b"") for _ in range(H // 6 + 40))     # keys are random: few are plausible
    items = [(ch[c][2] - 12, zeros) for c in two]
    out.append(Case("pool_dense", splice(wire, fo, items, rng), BIG_MF,
                    [("pool", c, w, "above") for c in two for w in ("wcap", "capc", "s0")] + [("pool", c, "d", "below") for c in two]))
    period = bytearray(b"\xff" * 96)
    for ph in range(0, 96, 16):
        period[ph:ph + 6] = bytes([0x82, 0x80 | 90, 0xFF, 0xFF, 0xFF, 0xFF])  # a frame of 96 B: the next one in its own phase
    body = bytes(period) * ((H + 2000) // 96) + b"\xff" * 300
    items = [(ch[c][2] - 50, frame(rng, len(body), body=body)) for c in two]
    out.append(Case("pool_exits", splice(wire, fo, items, rng), BIG_MF, [("pool", c, "d", "above") for c in two]))
    return out


THREE = dict(stream_split=80, stream_split2=160, stream_c0=0, stream_c1=0)


def handoff_cases():
    """three live parts: max_frames around each hand-off frame, bad headers at the chain's entry into parts 1 and 2"""
    wire, fo, fl = base_stream()
    g, P1, nf = geometry(wire, opts=THREE, fo=fo, fl=fl)
    ch = chunks_of(g)
    rng = np.random.default_rng(9400)
    bad = {"garbage": bytes([0x37, 0x91, 0xC3, 0x5A, 0x77, 0x13, 0xFE, 0x09, 0x44, 0xB2, 0x61, 0x0F, 0xA8, 0x3C]),
           "wrap": bytes([0x82, 0xFF]) + (0xFFFFFFFFFFFFFFF0).to_bytes(8, "big") + bytes(4),
           "unmasked": frame(rng, 30, masked=False), "rsv": frame(rng, 30, b0=0xC2)}
    out = []
    for k in (1, 2):
        i = int(np.searchsorted(fo, g.parts[k].P))               # the hand-off frame: in_nf = i
        for d in (-1, 0, 1):
            out.append(Case("max_handoff%d%+d" % (k, d), wire, i + d, [("max_at", "handoff%d" % k, d, i)], dict(THREE)))
        c = [j for j, x in enumerate(ch) if x[0] == k][0]
        for what, data in bad.items():
            w2 = wire.copy()
            w2[int(fo[i]):int(fo[i]) + len(data)] = np.frombuffer(data, dtype=np.uint8)
            out.append(Case("end_part%d_%s" % (k, what), w2, BIG_MF, [("end", c, "part%d" % k, what, int(fo[i]))], dict(THREE)))
    return out


def aligned_cases():
    """samples of their own, so that a cut (a whole 16 KiB piece) meets the chunk grid: a frame start exactly
    at 256 KiB (a cut on a chunk start), and a 16 KiB frame across 256 KiB that ends one byte before a piece
    (the cut one byte inside part 0's only chunk)"""
    wire, fo, fl = base_stream()
    rng = np.random.default_rng(9500)
    a = int(fo[np.searchsorted(fo, M.SAMPLE - 6, side="right") - 1])
    b = int(fo[np.searchsorted(fo, M.SAMPLE + 6)])
    w1 = wire.copy()
    w1[a:b] = np.frombuffer(filler(rng, M.SAMPLE - a) + filler(rng, b - M.SAMPLE), dtype=np.uint8)
    x1 = 20 * M.PIECE                                            # = 256 KiB + one chunk
    out = [Case("aligned_cut_on_chunk_start", w1, BIG_MF, [("split", "cut_on_chunk_start", x1)],
                dict(stream_split=64, stream_split2=0, stream_c0=0, stream_c1=0))]
    s0, P1 = M.SAMPLE - 4, M.SAMPLE + M.PIECE - 1
    a = int(fo[np.searchsorted(fo, s0 - 6, side="right") - 1])
    b = int(fo[np.searchsorted(fo, P1 + 6)])
    w2 = wire.copy()
    w2[a:b] = np.frombuffer(filler(rng, s0 - a) + _long_frame(rng, P1 - s0) + filler(rng, b - P1), dtype=np.uint8)
    out.append(Case("aligned_cut_one_byte_inside", w2, BIG_MF, [("split", "cut_one_byte_inside", 17 * M.PIECE)],
                    dict(stream_split=55, stream_split2=0, stream_c0=0, stream_c1=0)))
    return out


# ---- the pass loop (streams under 512 KiB, or uniform runs): parity cases, their claims about run lengths

def uniform(rng, n, plen):
    return b"".join(frame(rng, plen) for _ in range(n))


def pass_cases():
    """[(name, wire, max_frames, options, claim)]; claim: (leading run length, frames) checked on the oracle's lengths"""
    rng = np.random.default_rng(9600)
    tail = lambda k=40: b"".join(frame(rng, int(rng.integers(20, 91))) for _ in range(k))
    arr = lambda b: np.frombuffer(b, dtype=np.uint8).copy()
    out = []
    # pass A takes candidates [0, 4096): a run that ends at candidate 4095, 4096, 4097 (the length changes there)
    for n in (4095, 4096, 4097):
        out.append(("run_%d" % n, arr(uniform(rng, n, 20) + frame(rng, 33) + tail()), BIG_MF, {}, ("run", n)))
        out.append(("run_%d_then_run" % n, arr(uniform(rng, n, 20) + uniform(rng, 300, 7)), BIG_MF, {}, ("run", n)))
    # stream_rounds 1 and 4 with rounds - 1, rounds, rounds + 1 length changes (runs of 100 frames)
    for rounds in (1, 4):
        for changes in (rounds - 1, rounds, rounds + 1):
            w = b"".join(uniform(rng, 100, 10 + 7 * r) for r in range(changes + 1))
            out.append(("rounds%d_changes%d" % (rounds, changes), arr(w), BIG_MF, {"stream_rounds": rounds}, ("changes", changes)))
    # changing lengths at 512 KiB - 1, + 0, + 1 (the threshold between the one-wavefront walk and the chunk walk)
    base = base_stream()[0]
    for d in (-1, 0, 1):
        out.append(("len_512k%+d" % d, base[:(512 << 10) + d].copy(), BIG_MF, {}, ("len", (512 << 10) + d)))
    # a first frame that is incomplete, of zero length, or an error: only candidate 0 exists
    out.append(("first_incomplete", arr(frame(rng, 300)[:9]), 16, {}, ("frames", 0)))
    out.append(("first_zero", arr(frame(rng, 0) + tail(5)), 16, {}, ("frames", 6)))
    out.append(("first_wrap", arr(bytes([0x82, 0xFF]) + (0xFFFFFFFFFFFFFFF0).to_bytes(8, "big") + bytes(4) + tail(5)), 16, {}, ("frames", 0)))
    out.append(("first_only_byte", arr(b"\x82"), 16, {}, ("frames", 0)))
    return out


def rest_cases():
    """a rest after the sample of 255 and 256 mean frames (RW_MIN_FRAMES): frames of 1000-1200 B payloads so that
    the stream is still longer than 512 KiB; (wire, plan active)"""
    rng = np.random.default_rng(9700)
    w = np.frombuffer(b"".join(frame(rng, int(rng.integers(1000, 1201))) for _ in range(700)), dtype=np.uint8).copy()
    fo, fl, _ = frame_offsets(w)
    P1, nf, mean, _ = sample_of(fo, fl, len(w))
    out = []
    for frames, active in ((255, 0), (256, 1)):
        n = P1 + frames * mean + (mean - 1 if frames == 255 else 0)     # (len - P1) // mean == frames, at its upper / lower end
        assert n <= len(w) and n >= M.MIN_STREAM and (n - P1) // mean == frames
        out.append(("rest_%d" % frames, w[:n].copy(), BIG_MF, active))
    return out


def pass_b_case():
    """6-byte frames, about 12.6 MiB: pass B's grid (at most 8192 blocks of 256) takes a second grid-stride step"""
    rng = np.random.default_rng(9800)
    n = 8192 * 256 + 4096 + 5000
    one = np.frombuffer(frame(rng, 0), dtype=np.uint8)
    return np.tile(one, n), n


def host_walk_geometry(wire, fo=None, fl=None):
    """the model of an eager host-linked call (stream_rw 2) on a stream of changing lengths: the pass rounds
    first — each takes the run of equal frames at P and the frame of another length after it, and two rounds
    in a row that met the other length within 64 candidates hand over to the walk — then the sample from
    there and the host rule. Returns (Geom of one part, P1, frames before it, P the walk started at)"""
    if fo is None:
        fo, fl, _ = frame_offsets(wire)
    i, short = 0, 0
    while short < 2:
        m = 1
        while i + m < len(fl) and fl[i + m] == fl[i]:
            m += 1
        assert i + m < len(fl)
        i += m + 1
        if m < 64:
            short += 1
    P = int(fo[i])
    k = int(np.searchsorted(fo, P + M.SAMPLE))
    P1 = int(fo[k])
    mean = M.mean_of(P, P1, k - i)
    if M.short_rest(P1, len(wire), mean):
        return None
    C, H, n, stgn, capc = M.host_plan(P1, len(wire), mean, 1 << 22)
    empty = M.Part(len(wire), 0, 0, 0, n, 0, 0, 0, 0)
    return M.Geom([M.Part(P1, C, H, n, 0, capc, stgn, 0, 0), empty, empty], 1, n), P1, k, P


def grid_cases(ch, H, tag, seed):
    """the chunk-start and window cells on any chunk grid `ch` (chunks_of form) of the base stream: a frame
    at cs - 1, cs, cs + 1, a zero-length frame ending at cs, the chain's entry at cs + H - 1 and cs + H; at a
    middle chunk and the last"""
    wire, fo, fl = base_stream()
    rng = np.random.default_rng(seed)
    last = len(ch) - 1
    out = []
    for d in (-1, 0, 1):
        items = [(ch[c][2] + d, frame(rng, 40)) for c in (3, last)]
        out.append(Case("%s_start%+d" % (tag, d), splice(wire, fo, items, rng), BIG_MF, [("start", c, d) for c in (3, last)]))
    items = [(ch[c][2] - 6, frame(rng, 0) + frame(rng, 33)) for c in (5, last)]
    out.append(Case(tag + "_zero_end", splice(wire, fo, items, rng), BIG_MF, [("zero_end", c) for c in (5, last)]))
    for d in (H - 1, H):
        items = [(ch[c][2] - 40, _long_frame(rng, 40 + d) + frame(rng, 25)) for c in (6, last)]
        out.append(Case("%s_entry_%d" % (tag, d), splice(wire, fo, items, rng), BIG_MF, [("entry", c, d) for c in (6, last)]))
    return out


def host_cases():
    wire, fo, fl = base_stream()
    g, P1, nf, P = host_walk_geometry(wire, fo, fl)
    return grid_cases(chunks_of(g), g.parts[0].H, "host", 9900)


def seen_after(wire, max_frames=BIG_MF):
    """the longest frame a chunk walk from 0 writes after its sample: the next call's `seen`"""
    fo, fl, _ = frame_offsets(wire, max_frames)
    k = int(np.searchsorted(fo, M.SAMPLE))
    return int(fl[k:].max()) if k < len(fl) else 0


GROUPS = {"chunk_start": chunk_start_cases, "window_long": window_and_long_cases, "stream_end": stream_end_cases,
          "counts": count_cases, "endings": ending_cases, "splits": split_cases, "handoffs": handoff_cases,
          "aligned": aligned_cases, "pools": pool_cases}
_cases = {}


def cases(group):
    if group not in _cases:
        _cases[group] = GROUPS[group]()
    return _cases[group]
