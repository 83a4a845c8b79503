"""Directed inputs for websocketframeBatchDecodeDevice (tests/test_gpu_decode_edges.py) and a
classifier that says which kernel branches a batch reaches (tests/test_dec_cases.py).

Every builder takes lead0, the 16-byte phase of the buffer's base address (the kernels work in
"origin" coordinates = wire offset + lead0: 16 KiB pieces, 4 KiB wave ranges and 16-byte chunks
are aligned there), and returns (wire, seg_off, seg_len, max_frames); with with_plain=True a
fifth element, the buffer a decode of every frame leaves behind. Bytes outside the segments are
0xA5. CPU only: numpy and the oracle, no torch.
"""
import os
import re

import numpy as np

import wsynth
from oracle_lib import oracle_segments
from reasm_cases import frame as wire_frame

GAP = 0xA5
PIECE = 16384
WAVE = 4096
HLS = (2, 4, 6, 8, 10, 14)
SMALL_LENS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49)
RUN_N = (1, 2, 15, 16, 17, 31, 32, 33, 48)
RUN_ENDINGS = ("end", "other", "cut:1", "cut:5", "cut:6", "cut:7", "cut:36", "wrap")
RUN_MF = sorted({m for n in RUN_N for m in (n - 1, n, n + 1) if m} | {64})
ALPHA_MF = (1, 2, 3, 4, 5, 7, 13, 15, 16, 17)
LONG_PLEN = (1 << 20) + PIECE + 5
WRAP_HDR = bytes([0x82, 0xFF]) + b"\xff" * 8          # masked, 64-bit length 2^64 - 1: SEG_ERR_LEN_WRAP


def segfuse_w1():
    """bytes a segfuse window owns: (SF_L - 1) KiB, SF_L read from the kernel's launch"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "util_amd", "csrc", "ws_segfuse.hip")
    with open(src) as f:
        m = re.search(r"ws_segfuse_kernel<\s*\d+\s*,\s*(\d+)\s*,\s*\d+\s*>\)", f.read())
    return (int(m.group(1)) - 1) * 1024


W1 = segfuse_w1()


def fr(rng, plen, masked=True, form=None, b0=0x82):
    """one frame as (wire bytes, bytes after the decode)"""
    plen = int(plen)
    minimal = 7 if plen < 126 else (16 if plen <= 0xFFFF else 64)
    if masked and (form or minimal) == minimal:
        key = int(rng.integers(0, 1 << 32))
        body = rng.integers(0, 256, plen, dtype=np.uint8)
        h = wsynth.header(b0, plen, key).tobytes()
        kb = np.frombuffer(key.to_bytes(4, "little"), dtype=np.uint8)
        return h + (body ^ np.resize(kb, plen) if plen else body).tobytes(), h + body.tobytes()
    if not masked:
        w = wire_frame(rng, b0, plen, masked=False, form=form)
        return w, w
    w = wire_frame(rng, b0, plen, masked=True, form=form)
    hl = len(w) - plen
    body = np.frombuffer(w[hl:], dtype=np.uint8)
    key = np.frombuffer(w[hl - 4:hl], dtype=np.uint8)
    return w, w[:hl] + (body ^ np.resize(key, plen) if plen else body).tobytes()


def by_hdr(rng, hl, plen=None):
    """a frame whose header is hl bytes long (minimal length form: 10 and 14 carry 64 KiB)"""
    masked = hl in (6, 8, 14)
    plen = plen if plen is not None else {2: 100, 6: 100, 4: 300, 8: 300, 10: 65536, 14: 65536}[hl]
    f = fr(rng, plen, masked=masked)
    assert len(f[0]) == hl + plen
    return f


class Batch:
    def __init__(self, lead0=0):
        self.lead0 = lead0
        self.w, self.p, self.so, self.sl = bytearray(), bytearray(), [], []

    @property
    def x(self):
        """origin coordinate of the next byte"""
        return len(self.w) + self.lead0

    def gap(self, n):
        self.w += bytes([GAP]) * n
        self.p += bytes([GAP]) * n

    def gap_to(self, x):
        assert x >= self.x, (x, self.x)
        self.gap(x - self.x)

    def next_boundary(self, room=0):
        """the first piece boundary with at least `room` bytes of gap before it"""
        return -(-(self.x + room) // PIECE) * PIECE

    def seg(self, *parts):
        """one segment: frames (wire, plain) and raw bytes, back to back"""
        self.so.append(len(self.w))
        for f in parts:
            if isinstance(f, tuple):
                self.w += f[0]
                self.p += f[1]
            else:
                self.w += f
                self.p += f
        self.sl.append(len(self.w) - self.so[-1])

    def done(self, max_frames, with_plain=False):
        wire = np.frombuffer(bytes(self.w), dtype=np.uint8).copy()
        out = (wire, list(self.so), list(self.sl), max_frames)
        return out + (np.frombuffer(bytes(self.p), dtype=np.uint8).copy(),) if with_plain else out


def seglen(*parts):
    return sum(len(f[0]) if isinstance(f, tuple) else len(f) for f in parts)


# ---------------------------------------------------------------------------------- builders

def run_lengths(lead0=0, max_frames=64, with_plain=False):
    """one segment per (n, ending): n equal 37-byte frames, then the ending"""
    rng = np.random.default_rng(100)
    b = Batch(lead0)
    i = 0
    for n in RUN_N:
        for ending in RUN_ENDINGS:
            b.gap(i * 5 % 13 + 1)
            i += 1
            parts = [fr(rng, 31) for _ in range(n)]
            if ending == "other":
                parts.append(fr(rng, 50))
            elif ending.startswith("cut:"):
                parts.append(fr(rng, 31)[0][:int(ending[4:])])
            elif ending == "wrap":
                parts.append(WRAP_HDR + rng.integers(0, 256, 23, dtype=np.uint8).tobytes())
            b.seg(*parts)
    b.gap(3)
    return b.done(max_frames, with_plain)


def _a(rng):
    return fr(rng, 20)


def _b(rng):
    return fr(rng, 33)


def _c(rng):
    return fr(rng, 7)


def _d(rng):
    return fr(rng, 60)


def _e(rng):
    return fr(rng, 45, masked=False)


def _same(k):
    # 106 wire bytes each: masked 100 B, unmasked 104 B, masked 98 B in the 16-bit form
    return [lambda r: fr(r, 100), lambda r: fr(r, 104, masked=False), lambda r: fr(r, 98, form=16)][k]


_L = {"A": _a, "B": _b, "C": _c, "D": _d, "E": _e, "x": _same(0), "y": _same(1), "z": _same(2)}
PATTERNS = {
    "ABAB": "AB" * 20,
    "AABB": "AABB" * 10,
    "ABC": "ABC" * 13 + "A",
    "ABCD": "ABCD" * 10,
    "ABCDE": "ABCDE" * 8,
    "AAAB": "AAAB" * 10,
    "ABABAB8C": "ABABAB" + "C" * 8,
    "SAME": "xyz" * 14,
}
SWEEP_BYTES = 1400


def alphabets(lead0=0, pattern="ABAB", variant="full", max_frames=64, with_plain=False):
    """variant "full": the pattern and the pattern without its first frame, one segment each;
    "sweep": segment i holds the first i bytes of the pattern's first <= 1400 bytes, i = 0..len"""
    rng = np.random.default_rng(200 + sorted(PATTERNS).index(pattern))
    frames = [_L[ch](rng) for ch in PATTERNS[pattern]]
    b = Batch(lead0)
    if variant == "full":
        b.gap(5)
        b.seg(*frames)
        b.gap(7)
        b.seg(*frames[1:])
        b.gap(2)
        return b.done(max_frames, with_plain)
    assert variant == "sweep" and not with_plain
    head = b""
    for f in frames:
        if len(head) + len(f[0]) > SWEEP_BYTES:
            break
        head += f[0]
    for i in range(len(head) + 1):
        b.gap(i % 3)
        b.seg(head[:i])
    b.gap(1)
    return b.done(max_frames)


def sweep_frames(pattern):
    """the wire lengths of the frames in a sweep's pattern head"""
    wire, so, sl, mf = alphabets(0, pattern, "sweep")
    d, r = oracle_segments(wire[so[-1]:so[-1] + sl[-1]].copy(), [0], [sl[-1]], 64)
    return [int(x) for x in d["ret"][:int(r[0]["n_frames"])]]


def piece_edges(lead0=0, variant="short", with_plain=False):
    """variant "short": headers of 2/4/6/8 bytes split at every byte over a piece boundary, payload
    starting on it, frame ending on it (the frame second in its segment), then a boundary inside
    gaps of 1 / 17 / 40 bytes, a garbage tail, a truncated last frame, frames left unwalked by
    MAX_FRAMES (4), an unmasked frame, three zero-length segments: each followed, in the same
    piece, by a segment of masked frames. "long": the 10- and 14-byte headers (64 KiB payloads)"""
    rng = np.random.default_rng(300 + (variant == "long"))
    b = Batch(lead0)
    for hl in ((2, 4, 6, 8) if variant == "short" else (10, 14)):
        for k in list(range(1, hl + 1)) + ["end"]:            # k == hl: the payload starts on the boundary
            pre, f, post = fr(rng, 20), by_hdr(rng, hl), fr(rng, 9)
            back = len(pre[0]) + (len(f[0]) if k == "end" else k)
            bd = b.next_boundary(back + 1)
            b.gap_to(bd - back)
            b.seg(pre, f, post)
            assert (b.so[-1] + lead0 + len(pre[0]) + (len(f[0]) if k == "end" else k)) % PIECE == 0
    if variant == "long":
        b.gap(11)
        return b.done(4, with_plain)

    def follower():
        return [fr(rng, 40), fr(rng, 300), fr(rng, 3)]

    for g, before in ((1, 0), (17, 8), (40, 20)):              # the boundary `before` bytes into a g-byte gap
        first = [fr(rng, 70), fr(rng, 33)]
        bd = b.next_boundary(seglen(*first) + before + 1)
        b.gap_to(bd - before - seglen(*first))
        b.seg(*first)
        b.gap(g)
        b.seg(*follower())
    # garbage tail, truncated last frame, MAX_FRAMES leftovers, unmasked frame: boundary 30 bytes in
    tails = [
        ([fr(rng, 25), fr(rng, 60)], WRAP_HDR + rng.integers(0, 256, 90, dtype=np.uint8).tobytes()),
        ([fr(rng, 25), fr(rng, 60)], fr(rng, 500)[0][:200]),
        ([fr(rng, 25), fr(rng, 60), fr(rng, 5), fr(rng, 0)], b"".join(fr(rng, 30)[0] for _ in range(6))),
        ([fr(rng, 25)], b"".join(x[0] for x in (fr(rng, 300, masked=False), fr(rng, 44)))),
    ]
    for head, tail in tails:
        bd = b.next_boundary(seglen(*head) + 31)
        b.gap_to(bd - 30 - seglen(*head))
        b.seg(*head, tail)
        assert b.so[-1] + lead0 + seglen(*head) + 30 == bd
        b.gap(3)
        b.seg(*follower())
    # three zero-length segments around a boundary
    bd = b.next_boundary(60)
    b.gap_to(bd - 50)
    b.seg(fr(rng, 30))
    b.gap_to(bd - 3)
    b.seg()
    b.gap(3)
    b.seg()
    b.gap(5)
    b.seg()
    b.gap(4)
    b.seg(*follower())
    b.gap(9)
    out = b.done(4, with_plain)
    if with_plain:                                            # the plain image holds only for walked frames
        out = out[:4] + (None,)
    return out


def small_payloads(lead0=0, with_plain=False):
    """two frames per segment: an unmasked filler of 0-15 bytes, then a masked / unmasked frame of
    each small payload length with its payload at each of the 16 chunk phases; segments back to
    back or one byte apart"""
    rng = np.random.default_rng(400)
    b = Batch(lead0)
    b.gap(3)
    i = 0
    for ph in range(16):
        for masked in (1, 0):
            for plen in SMALL_LENS:
                hl = 6 if masked else 2
                fill = (ph - b.x - 2 - hl) % 16
                b.seg(fr(rng, fill, masked=False), fr(rng, plen, masked=bool(masked)))
                b.gap(1 if i % 3 == 1 else 0)
                i += 1
    b.gap(5)
    return b.done(2, with_plain)


TINY = ((0, False), (0, True), (1, True), (2, True), (3, True))       # 2, 6, 7, 8, 9 wire bytes
DENSE_COUNTS = (15, 16, 17, 80, 81, 150, 16, 33)


def dense_items(lead0=0, variant="frames", with_plain=False):
    """"frames" (max_frames 4096) / "frames64" (the same bytes, max_frames 64): one segment; from
    each piece boundary on N - 1 tiny frames, then one frame that ends on the next boundary, N in
    DENSE_COUNTS: wave range 0 of the piece scans N items, the next piece's first item is N later.
    "segments": ~600 one-frame segments of 10-20 bytes, empty and garbage-only ones among them"""
    rng = np.random.default_rng(500)
    b = Batch(lead0)
    if variant == "segments":
        b.gap(2)
        for i in range(600):
            if i % 11 == 4:
                b.seg()
            elif i % 13 == 7:
                b.seg(WRAP_HDR[:int(rng.integers(1, 11))])
            else:
                b.seg(fr(rng, int(rng.integers(4, 15))))
            b.gap((0, 1, 0, 3)[i % 4])
        b.gap(6)
        return b.done(2, with_plain)
    bd = b.next_boundary(1)
    b.gap_to(bd)
    parts, x, t = [], bd, 0
    for n in DENSE_COUNTS:
        for _ in range(n - 1):
            plen, masked = TINY[t % len(TINY)]
            t += 1
            parts.append(fr(rng, plen, masked=masked))
            x += len(parts[-1][0])
        bd += PIECE
        parts.append(fr(rng, bd - x - 8))                     # 16-bit form: 8-byte header
        x = bd
    parts += [fr(rng, 2), fr(rng, 0, masked=False), fr(rng, 3)]
    b.seg(*parts)
    b.gap(4)
    out = b.done(4096 if variant == "frames" else 64, with_plain)
    return out[:4] + (None,) if with_plain and variant != "frames" else out


def long_not_first(lead0=0, with_plain=False):
    """a frame of more than 64 pieces that is not its segment's first: after three equal frames
    (a stride lane), after A B A and after A B A B (alphabet lanes of depth 1 and 2); two small
    frames after it"""
    rng = np.random.default_rng(600)
    b = Batch(lead0)
    for lead in ("AAA", "ABA", "ABAB"):
        b.gap(7 if lead == "AAA" else 13)
        b.seg(*([_L[ch](rng) for ch in lead] + [fr(rng, LONG_PLEN), fr(rng, 12), fr(rng, 5)]))
    b.gap(3)
    return b.done(8, with_plain)


SF_OFFSETS = tuple(range(-14, 2))


def segfuse_windows(lead0=0, variant="edges", with_plain=False):
    """"edges" (max_frames 4): a header of each size starting at each offset in [W1 - 14, W1 + 1] of
    its segment's first window (the 10- and 14-byte headers in the non-minimal 64-bit form over a
    short payload, which the decode accepts), a frame ending exactly at W1, a 40 KiB unmasked frame
    followed by masked frames. "run64" (max_frames 64): 64 and 65 equal tiny frames"""
    rng = np.random.default_rng(700)
    b = Batch(lead0)
    if variant == "run64":
        for n in (64, 65):
            b.gap(5)
            b.seg(*[fr(rng, 3) for _ in range(n)])
        b.gap(2)
        out = b.done(64, with_plain)
        return out[:4] + (None,) if with_plain else out       # the 65th frame stays masked
    for hl in HLS:
        for d in SF_OFFSETS:
            b.gap(1 + (d & 3))
            lead = b.x & 15
            pos = W1 + d - lead                                # segment-relative header start
            tgt = fr(rng, 300, masked=hl == 14, form=64) if hl >= 10 else by_hdr(rng, hl)
            b.seg(fr(rng, pos - 8), tgt, fr(rng, 21))
    b.gap(3)
    lead = b.x & 15
    b.seg(fr(rng, W1 - lead - 8), fr(rng, 50))
    b.gap(6)
    b.seg(fr(rng, 18), fr(rng, 40 << 10, masked=False), fr(rng, 100), fr(rng, 2000))
    b.gap(2)
    return b.done(4, with_plain)


GEOMETRIC = {"piece_edges", "small_payloads", "dense_items", "long_not_first", "segfuse_windows"}   # wire depends on lead0


def catalogue():
    """[(id, builder, kwargs, max_frames values to run it with)]; the builder's own max_frames first"""
    out = [("run_lengths", run_lengths, {}, [64] + [m for m in RUN_MF if m != 64])]
    for p in PATTERNS:
        out.append(("alphabets:%s:full" % p, alphabets, {"pattern": p, "variant": "full"}, [64] + list(ALPHA_MF)))
        out.append(("alphabets:%s:sweep" % p, alphabets, {"pattern": p, "variant": "sweep"}, [64]))
    out += [("piece_edges:short", piece_edges, {"variant": "short"}, [4]),
            ("piece_edges:long", piece_edges, {"variant": "long"}, [4]),
            ("small_payloads", small_payloads, {}, [2]),
            ("dense_items:frames", dense_items, {"variant": "frames"}, [4096]),
            ("dense_items:frames64", dense_items, {"variant": "frames64"}, [64]),
            ("dense_items:segments", dense_items, {"variant": "segments"}, [2]),
            ("long_not_first", long_not_first, {}, [8]),
            ("segfuse_windows:edges", segfuse_windows, {"variant": "edges"}, [4]),
            ("segfuse_windows:run64", segfuse_windows, {"variant": "run64"}, [64])]
    return out


def shifts_of(cid):
    return tuple(range(16)) if cid.split(":")[0] in ("small_payloads", "piece_edges") else (0, 1, 8, 15)


# ---------------------------------------------------------------------------------- classifier

def _letters(lens):
    seen = {}
    return "".join(chr(65 + min(seen.setdefault(x, len(seen)), 25)) for x in lens)


def features(wire, seg_off, seg_len, max_frames, lead0):
    """the cells a batch reaches, from the oracle's descriptors and segment results alone"""
    desc, res = oracle_segments(np.asarray(wire, dtype=np.uint8).copy(), seg_off, seg_len, max_frames)
    return features_of(desc, res, seg_off, seg_len, max_frames, lead0, len(wire))


def features_of(desc, res, seg_off, seg_len, max_frames, lead0, nbytes):
    out = set()
    nseg = len(seg_off)
    so = np.asarray(seg_off, dtype=np.int64) + lead0             # origin coordinates from here on
    sl = np.asarray(seg_len, dtype=np.int64)
    end = so + sl
    ordered = bool(nseg == 0 or ((so[1:] >= end[:-1]).all()))
    segs = []                                                 # per segment: fo, p0, fe, masked, plen, hl
    for s in range(nseg):
        nf, st = int(res[s]["n_frames"]), int(res[s]["status"])
        d = desc[s * max_frames:s * max_frames + nf]
        fo = d["frame_off"].astype(np.int64) + lead0
        hl = d["hdrlen"].astype(np.int64)
        ln = d["ret"].astype(np.int64)
        fe, p0 = fo + ln, fo + hl
        m, plen = d["masked"] != 0, d["datalen"].astype(np.int64)
        segs.append((fo, p0, fe, m, plen, hl))
        out.add("status:%d" % st)
        consumed = int(res[s]["consumed"])
        rem = int(sl[s]) - consumed
        lens = [int(x) for x in ln]
        run = 0
        while run < nf and lens[run] == lens[0]:
            run += 1
        kind = "max_frames" if st == 1 else ("wrap" if st == -2 else ("end" if rem == 0 else "incomplete"))
        if nf and nf - run <= 1:
            if kind == "end":
                out.add("run:%d:%s" % (run, "end" if nf == run else "other"))
            elif nf == run:
                out.add("run:%d:%s" % (run, "cut:%d" % rem if kind == "incomplete" else kind))
        lt = _letters(lens)
        out.add("stop:%s:%s" % (kind, lt[:17]))
        if nf >= 14:
            for p in range(1, 6):
                if all(lt[i] == lt[i - p] for i in range(p, nf)):
                    out.add("seq:period:" + lt[:p])
                    break
            else:
                if re.fullmatch(r"(AB){3}C{8}", lt):
                    out.add("seq:ABABAB8C")
        if nf >= 2 and ((ln[1:] == ln[:-1]) & ((hl[1:] != hl[:-1]) | (m[1:] != m[:-1]))).any():
            out.add("same_len_diff_hdr")
        for j in range(nf):
            a, h, e, q = int(fo[j]), int(hl[j]), int(fe[j]), int(p0[j])
            bd = (a // PIECE + 1) * PIECE
            if bd < a + h:
                out.add("hdr%d_split%d" % (h, bd - a))
            if q % PIECE == 0:
                out.add("payload_on_boundary:hdr%d" % h)
            if e % PIECE == 0:
                out.add("frame_end_on_boundary:hdr%d" % h)
            if int(plen[j]) in SMALL_LENS:
                out.add("small:%s:%d:ph%d" % ("m" if m[j] else "u", int(plen[j]), q & 15))
            lead = int(so[s]) & 15                            # segfuse: first-window coordinates
            x = a - int(so[s]) + lead
            if -14 <= x - W1 <= 1:
                out.add("sf_hdr%d:%d" % (h, x - W1))
                if x < W1 < x + h:
                    out.add("sf_straddle%d:%d" % (h, W1 - x))
            if e - int(so[s]) + lead == W1:
                out.add("sf_frame_end_at_W1")
            if j and (e + PIECE - 1) // PIECE - (a + PIECE - 1) // PIECE > 64:
                out.add("long_not_first:" + lt[:j])
            if not m[j] and e - a >= (40 << 10) and nf <= 64 and (m[j + 1:] & (plen[j + 1:] > 0)).any():
                out.add("sf_unmasked_jump")
    if not ordered:
        return out | {"unordered"}
    has_masked = [bool((g[3] & (g[4] > 0)).any()) for g in segs]
    for s in range(nseg - 1):
        g = int(so[s + 1] - end[s])
        if g in (0, 1) and end[s] & 15 and sl[s] and sl[s + 1] and has_masked[s] and has_masked[s + 1]:
            out.add("seg_adjacent:gap%d" % g)

    def masked_follows(s_from, bd):
        """a later segment has a masked payload starting inside the piece [bd, bd + PIECE)"""
        for t in range(s_from, nseg):
            if so[t] >= bd + PIECE:
                return False
            fo, p0, fe, m, plen, hl = segs[t]
            if (m & (plen > 0) & (p0 >= bd) & (p0 < bd + PIECE)).any():
                return True
        return False

    nonempty = np.nonzero(sl > 0)[0]
    ptrs = []                                                 # (piece boundary, segment, item) as K1 points them
    for bd in range(0, lead0 + nbytes, PIECE):                # piece 0 starts lead0 bytes before the buffer
        s = int(np.searchsorted(end, bd, side="right"))
        if s >= nseg:
            ptrs.append((bd, None, None))
            continue
        fo, p0, fe, m, plen, hl = segs[s]
        nf = len(fo)
        if bd < lead0:
            k = 0
            if masked_follows(0, bd):
                out.add("piece_first_byte_in:before_buf")
        elif bd < so[s]:
            k = 0
            # the whole gap between the non-empty segments around bd, and the empty ones in it
            i = int(np.searchsorted(end[nonempty], bd, side="right"))
            lo = int(end[nonempty[i - 1]]) if i else lead0
            hi = int(so[nonempty[i]]) if i < len(nonempty) else lead0 + nbytes
            nxt = int(nonempty[i]) if i < len(nonempty) else nseg
            empties = so[(sl == 0) & (so >= lo) & (so <= hi)]
            if masked_follows(nxt, bd):
                if len(empties) >= 3 and (empties <= bd).any() and (empties > bd).any():
                    out.add("piece_first_byte_in:empty_seg")
                elif len(empties) == 0:
                    out.add("piece_first_byte_in:gap")
                    out.add("piece_gap:%d" % (hi - lo))
        elif bd >= so[s] + int(res[s]["consumed"]):
            k = nf
            if masked_follows(s + 1, bd):
                out.add("piece_first_byte_in:tail")
                out.add("piece_tail:status%d" % int(res[s]["status"]))
        else:
            k = int(np.searchsorted(fo, bd, side="right")) - 1
            where = "header" if bd < p0[k] else ("payload" if m[k] else "unmasked")
            if where == "payload" or masked_follows(s + 1, bd):
                out.add("piece_first_byte_in:" + where)
        ptrs.append((bd, s, k))
    for i, (bd, s, k) in enumerate(ptrs):
        if s is None:
            continue
        nb, ns, nk = ptrs[i + 1] if i + 1 < len(ptrs) else (None, None, None)
        same = ns == s
        if same and nk - k in (15, 16, 17):
            out.add("ptr_delta:%d" % (nk - k))
        exact = same and 0 <= nk - k < 16
        p0 = segs[s][1]
        for w in range(4):
            r1 = bd + (w + 1) * WAVE
            n = int(np.searchsorted(p0, r1, side="left")) - k   # items from k on that start before r1
            if not exact:
                if n in (16, 17, 80, 81):
                    out.add("wave_items:%d" % n)
                elif n >= 145:
                    out.add("wave_items:145+")
            hops = int(np.searchsorted(so, r1, side="left")) - s
            if hops > 16:
                out.add("wave_segments:17+")
    return out
