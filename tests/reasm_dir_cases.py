"""Directed inputs for websocketframeBatchReassembleDevice(Ex/Ctl) (tests/test_gpu_reasm_edges.py)
and a classifier that says which cells of util_amd/csrc/ws_reasm.hip a batch reaches
(tests/test_reasm_dir_cases.py).

Every builder takes bw and bo, the 16-byte phases of the wire and output buffers' base addresses,
and returns a Case: (wire, seg_off, seg_len, max_frames, kwargs), kwargs carrying open_in,
cached_in, readcache_max, out_off, out_size and flags (and buflen for the dispatch corners);
Case.frames[s] lists the frames the builder wrote into segment s as (first byte, plaintext body).
Bytes outside the segments are 0xA5. CPU only: numpy and the oracle, no torch.

features(case, L) replays, from the oracle's output alone, the geometry of both implementations:
the fused kernel's windows (lead = (bw + seg_off) & 15, W0 = 0, W1 = W0 + (L-1) KiB, the next W0 =
W1 while the last placed body ends past W1, else floor16(off + lead)), its walk rounds (a run of
up to 64 frames of one wire length plus the frame that changes the length), and the layout
kernel's rounds of RLAY_G frames. L, RLAY_G and RSEG_TB are read from ws_reasm.hip, so a geometry
change moves the cases instead of silently testing the wrong bytes.
"""
import os
import re

import numpy as np

from oracle_lib import oracle_reassemble
from reasm_ctl_oracle import oracle_reassemble_ctl

CTL = 1                                                   # WEBSOCKET_REASM_CONTROL_DIRECT
GAP = 0xA5
HLS = (2, 4, 6, 8, 10, 14)
EDGE_D = (1, 15, 16)
COPY_LENS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 1023, 1024, 1025, 1039, 1040, 1041)
SEG_FRAMES = (15, 16, 17, 63, 64, 65, 200, 260)
MFS_BOTH = (1, 15, 16, 17, 63, 64)
MFS_THREE = (65, 200)
U32_CACHED = ((1 << 32) - 16, (1 << 32) - 1)
U32_LIMITS = (0, 1, 100, (1 << 32) - 1)
U32_LENS = tuple(range(1, 41))
AUTO_CORNERS = tuple((n, m, p) for n in (1023, 1024) for m in (64, 65) for p in (0, 1))
BASES = ((0, 0), (5, 11))                                 # (wire, output) base phases the GPU test uses


def geometry():
    """(the fused kernel's window lengths L, RLAY_G, RSEG_TB) as ws_reasm.hip has them"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "util_amd", "csrc", "ws_reasm.hip")
    with open(src) as f:
        text = f.read()
    ls = sorted({int(x) for x in re.findall(r"ws_reasm_seg_kernel<\s*(\d+)\s*,", text)})
    g = int(re.search(r"#define\s+RLAY_G\s+(\d+)", text).group(1))
    tb = int(re.search(r"#define\s+RSEG_TB\s+(\d+)", text).group(1))
    return tuple(ls), g, tb


LS, RLAY_G, RSEG_TB = geometry()


class Frame:
    """w: wire bytes, b0: first byte, plain: the body before masking (None: the length-wrap quirk)"""

    def __init__(self, w, b0, plain):
        self.w, self.b0, self.plain = w, b0, plain


def fr(rng, plen, b0=0x82, masked=True, hl=None):
    """one frame with an hl-byte header (default: the minimal form); keys have four distinct bytes"""
    plen = int(plen)
    form = {2: 7, 4: 16, 10: 64}[hl - (4 if masked else 0)] if hl else (7 if plen < 126 else (16 if plen <= 0xFFFF else 64))
    h = bytearray([b0])
    m = 0x80 if masked else 0
    if form == 7:
        assert plen < 126
        h.append(m | plen)
    elif form == 16:
        assert plen <= 0xFFFF
        h += bytes([m | 126]) + plen.to_bytes(2, "big")
    else:
        h += bytes([m | 127]) + plen.to_bytes(8, "big")
    plain = rng.integers(0, 256, plen, dtype=np.uint8)
    body = plain
    if masked:
        key = rng.permutation(256)[:4].astype(np.uint8)
        h += key.tobytes()
        body = plain ^ np.resize(key, plen) if plen else plain
    return Frame(bytes(h) + body.tobytes(), b0, plain)


def quirk(b0=0x82):
    """an unmasked frame of length 2^64 - 1: 10 + length wraps to 9, so the reactor consumes 9 bytes
    and the next frame starts at the header's last byte, 0xFF (websocketframe.c:149); its body is
    larger than any region: WEBSOCKET_SEG_ERR_OUT_SPACE. The frame after it must have b0 = 0xFF."""
    return Frame(bytes([b0, 127]) + b"\xff" * 7, b0, None)


class Case(tuple):
    def __new__(cls, wire, so, sl, mf, kwargs, frames):
        t = tuple.__new__(cls, (wire, so, sl, mf, kwargs))
        t.frames = frames
        return t


class Batch:
    def __init__(self, bw=0, bo=0):
        self.bw, self.bo = bw, bo
        self.w, self.so, self.sl, self.frames = bytearray(), [], [], []
        self.open, self.cached, self.dph = [], [], []

    @property
    def x(self):
        return len(self.w) + self.bw

    def gap(self, n):
        self.w += bytes([GAP]) * n

    def lead(self, l):
        """1..16 gap bytes, so that the next segment's first byte has address phase l"""
        self.gap((l - self.x - 1) % 16 + 1)

    def seg(self, *frames, open_in=0, cached_in=0, dph=None):
        self.so.append(len(self.w))
        for f in frames:
            self.w += f.w
        self.sl.append(len(self.w) - self.so[-1])
        self.frames.append(list(frames))
        self.open.append(open_in)
        self.cached.append(cached_in)
        self.dph.append(dph)

    def done(self, mf, readcache_max=0, flags=0, out="own", perm=None, **extra):
        """out: "own" regions at the segments' own offsets (plus slack for a requested phase),
        "reverse": regions in reverse order with odd gaps"""
        self.gap(3)
        wire = np.frombuffer(bytes(self.w), dtype=np.uint8).copy()
        n = len(self.so)
        order = list(range(n)) if perm is None else list(perm)
        so, sl = [self.so[i] for i in order], [self.sl[i] for i in order]
        out_off, o = [0] * n, 5
        for s in (reversed(range(n)) if out == "reverse" else range(n)):
            want = self.dph[order[s]]
            if out == "reverse":
                o += 1 + 2 * (s % 4)                                   # odd gaps
            if want is not None:
                o += (want - self.bo - o) % 16
            out_off[s] = o
            o += sl[s]
        kw = dict(open_in=[self.open[i] for i in order], cached_in=[self.cached[i] for i in order],
                  readcache_max=readcache_max, out_off=out_off, out_size=o + 16, flags=flags)
        kw.update(extra)
        return Case(wire, so, sl, mf, kw, [self.frames[i] for i in order])


def oracle(case, mf=None, flags=None):
    """the checker's output for a case: (desc, res, msgs, regions, open_out, cached_out)"""
    wire, so, sl, mf0, kw = case
    fn = oracle_reassemble_ctl if (kw["flags"] if flags is None else flags) else oracle_reassemble
    return fn(wire, so, sl, mf or mf0, kw["open_in"], kw["out_off"], kw["readcache_max"], kw["cached_in"])


# ---------------------------------------------------------------------------------- builders

def by_hdr(rng, h, b0, plen=None):
    masked = h in (6, 8, 14)
    return fr(rng, plen if plen is not None else (40 if h in (2, 6) else 300), b0=b0, masked=masked, hl=h)


def windows(L, bw=0, bo=0):
    """max_frames 4. One segment per edge cell and window index w = 0, 1, 2: a filler frame whose
    body runs from the segment's start over w window edges (so the windows stay on multiples of
    (L-1) KiB), the target frame placed against the edge of window w, a control frame after it.
    Then bodies crossing 1, 2 and 3 edges, and per phase 1..15 a segment whose bodies stop at a
    length-wrap frame and whose next header lies that many bytes past the first edge."""
    rng = np.random.default_rng(1000 + L)
    wb = (L - 1) * 1024
    b = Batch(bw, bo)
    leads = (0, 1, 15, 7, 8)
    b0s = (0x00, 0x80, 0x89, 0x02, 0x8A)
    cnt = [0]

    def seg(w, back, target):
        """the target's header starts `back` bytes before the edge of window w"""
        lead = leads[cnt[0] % len(leads)]
        cnt[0] += 1
        b.lead(lead)
        pos = (w + 1) * wb - back - lead
        b.seg(fr(rng, pos - 8, b0=0x02, hl=8), target, fr(rng, 21, b0=0x8A))

    def b0():
        return b0s[cnt[0] % len(b0s)]

    for w in (0, 1, 2):
        for h in HLS:
            for k in range(0, h + 1):                      # 0: header at the edge, h: payload at the edge
                seg(w, k, by_hdr(rng, h, b0()))
        for d in EDGE_D:
            seg(w, 6 + 100 - d, fr(rng, 100, b0=b0()))      # body ends d bytes past the edge
            seg(w, 6 + d, fr(rng, 100, b0=b0()))            # body starts d bytes before it
    for i, n in enumerate((wb, 2 * wb + 50, 3 * wb + 70)):
        b.lead(leads[i])
        b.seg(fr(rng, 20, b0=0x02), fr(rng, n, b0=0x80, masked=i != 1), fr(rng, 9, b0=0x89))
    for ph in range(1, 16):
        lead = leads[ph % len(leads)]
        b.lead(lead)
        # quirk (9 bytes consumed), a frame from the 0xFF on that ends ph bytes past the edge, two more
        b.seg(quirk(), fr(rng, wb + ph - lead - 17, b0=0xFF, hl=8), fr(rng, 30, b0=0x80), fr(rng, 5, b0=0x89))
    return b.done(4)


def copy_phases(bw=0, bo=0):
    """max_frames 21. One segment per (source phase, destination phase, m) of its first body: 21
    adjacent bodies, one of each length of COPY_LENS, masked and unmasked in turn (m: which first).
    Body j's phases are the first body's plus fixed sums, so over the 256 starts every body meets
    every (source, destination) phase; the destination phase comes from out_off."""
    rng = np.random.default_rng(2000)
    b = Batch(bw, bo)
    order = (1040, 0, 17, 1, 1023, 33, 2, 1025, 47, 3, 16, 1039, 4, 49, 5, 1024, 15, 31, 1041, 32, 48)
    assert sorted(order) == sorted(COPY_LENS)
    for m in (0, 1):
        for sp in range(16):
            for dp in range(16):
                masked0 = m == 0
                b.lead((sp - (8 if masked0 else 4)) % 16)
                b.seg(*[fr(rng, n, b0=0x80 if j % 5 == 4 else 0x00, masked=(j + m) % 2 == 0) for j, n in enumerate(order)],
                      dph=dp)
    return b.done(len(order))


def ctl_bodies(bw=0, bo=0):
    """max_frames 8, flag CONTROL_DIRECT. Control bodies at every destination phase (packed downward
    from the region's end), of length zero, first, last and between every pair of the fragments of
    a message, as the last frame taken before max_frames, and the length-wrap frame with a control
    opcode (WEBSOCKET_SEG_ERR_OUT_SPACE)."""
    rng = np.random.default_rng(3000)
    b = Batch(bw, bo)
    for i, n in enumerate((1, 5, 16, 17, 33, 125, 1040, 2) * 2):        # the region's end = out_off + seg_len
        b.lead(i % 16)
        fs = [fr(rng, 30, b0=0x02), fr(rng, n, b0=0x89, masked=i % 3 != 0), fr(rng, 12, b0=0x80)]
        b.seg(*fs, dph=(i - sum(len(f.w) for f in fs) + n) % 16)
    b.lead(3)
    b.seg(fr(rng, 7, b0=0x01), fr(rng, 0, b0=0x89), fr(rng, 0, b0=0x8A, masked=False), fr(rng, 7, b0=0x80))
    frag = lambda k: fr(rng, 20 + k, b0=(0x02 if k == 0 else 0) | (0x80 if k == 3 else 0))  # noqa: E731
    for p in range(5):                                                   # one control frame at position p
        parts = [frag(k) for k in range(4)]
        parts.insert(p, fr(rng, 9, b0=0x89))
        b.lead(5 + p)
        b.seg(*parts)
    b.lead(11)                                                           # a control frame in every gap
    b.seg(fr(rng, 3, b0=0x8A), frag(0), fr(rng, 4, b0=0x89), frag(1), fr(rng, 0, b0=0x8A), frag(2), fr(rng, 6, b0=0x89), frag(3))
    b.lead(12)                                                           # frame 7 (taken) and frame 8 (not) are control
    b.seg(*([frag(0)] + [fr(rng, 5, b0=0x00) for _ in range(6)] + [fr(rng, 8, b0=0x89), fr(rng, 8, b0=0x8A), frag(3)]))
    b.lead(13)
    b.seg(fr(rng, 10, b0=0x02), quirk(0x89), fr(rng, 14, b0=0xFF), fr(rng, 3, b0=0x80))
    return b.done(8, flags=CTL)


def _eq(rng, b0, size):
    """a frame of `size` wire bytes: 14 (masked, 8-byte body) or 9 (masked, 3-byte body)"""
    return fr(rng, size - 6, b0=b0)


def round_edges(event, bw=0, bo=0):
    """max_frames 64. Segments of frames of one wire length (one walk round of the fused kernel,
    rounds of RLAY_G frames of the layout kernel) with the event at frame 0, RLAY_G - 1, RLAY_G,
    2 RLAY_G - 1, 2 RLAY_G, RSEG_TB - 1, and at frame 2 after a frame of another length (lane 0 of
    the fused walk's second round); each also with a message carried in (open_in 1, cached_in > 0).
    event "fin": the FIN frame that closes a message spanning a round edge; "refused": the frame
    the cache limit (7 bytes) refuses; "outspace": the first out-of-space body."""
    rng = np.random.default_rng(4000 + len(event))
    b = Batch(bw, bo)
    G, TB = RLAY_G, RSEG_TB
    size = 9 if event == "outspace" else 14
    ks = (0, G - 1, G, 2 * G - 1, 2 * G, TB - 1)
    i = 0
    for carry in (0, 1):
        for k in ks + ("B",):
            other = k == "B"                               # frame 0 of another length, event at frame 2
            kk = 2 if other else k
            fs = []
            for j in range(TB):
                if event == "fin":
                    b0 = 0x80 if j == kk or (j > kk and j % 7 == 3) else 0x00
                elif event == "refused":                   # FIN frames with nothing pending skip the check
                    b0 = 0x00 if j == kk else 0x80
                else:
                    b0 = 0x80 if j % 5 == 2 else 0x00
                f = _eq(rng, b0, size)
                if event == "refused" and carry and j == 0 and kk > 0:
                    f = fr(rng, 0, b0=0x80, hl=14)         # closes the carried message: 0 more bytes fit
                if other and j == 0:
                    f = fr(rng, 0, b0=0x80) if (event == "refused" and carry) else fr(rng, size - 4, b0=f.b0)
                if event == "outspace" and j == kk:
                    f = quirk(b0)
                elif event == "outspace" and j == kk + 1:
                    f = _eq(rng, 0xFF, size)
                fs.append(f)
            if event == "outspace" and kk == TB - 1:
                fs.append(Frame(b"\xff", 0xFF, None))      # the quirk header's tenth byte: an incomplete tail
            b.lead((3 * i) % 16)
            i += 1
            b.seg(*fs, open_in=carry, cached_in=2 * carry)
    return b.done(64, readcache_max=7 if event == "refused" else 0)


def frame_counts(bw=0, bo=0):
    """segments of 15, 16, 17, 63, 64, 65, 200 and 260 frames of one wire length, FIN on every fifth; run
    with every max_frames of MFS_BOTH and MFS_THREE"""
    rng = np.random.default_rng(5000)
    b = Batch(bw, bo)
    for i, n in enumerate(SEG_FRAMES):
        b.lead(2 * i + 1)
        b.seg(*[fr(rng, 8, b0=0x80 if j % 5 == 4 else (0x89 if j % 11 == 6 else 0x00)) for j in range(n)])
    return b.done(64)


def carry_first(bw=0, bo=0):
    """max_frames 8, flag CONTROL_DIRECT: a message carried in (open_in 1, cached_in 77) and the
    segment's first frame FIN, non-FIN, control, or absent (empty segment, one byte, a cut header)"""
    rng = np.random.default_rng(6000)
    b = Batch(bw, bo)
    segs = [[fr(rng, 10, b0=0x80), fr(rng, 4, b0=0x02)], [fr(rng, 10, b0=0x00)],
            [fr(rng, 6, b0=0x89), fr(rng, 10, b0=0x00), fr(rng, 3, b0=0x8A)], [],
            [Frame(b"\x82", 0x82, None)], [Frame(fr(rng, 300, b0=0x82).w[:5], 0x82, None)]]
    for i, fs in enumerate(segs):
        b.lead(4 * i + 2)
        b.seg(*fs, open_in=1, cached_in=77)
    return b.done(8, flags=CTL)


def u32_cached(limit, bw=0, bo=0):
    """max_frames 4: cached_in 2^32 - 16 and 2^32 - 1, a non-FIN frame of 1..40 bytes, a FIN frame"""
    rng = np.random.default_rng(7000)
    b = Batch(bw, bo)
    for c in U32_CACHED:
        for n in U32_LENS:
            b.lead(n % 16)
            b.seg(fr(rng, n, b0=0x00), fr(rng, 2, b0=0x00), fr(rng, 1, b0=0x80), open_in=1, cached_in=c)
    return b.done(4, readcache_max=limit)


def layout(bw=0, bo=0):
    """max_frames 8: segments in permuted order, zero-length segments first, in the middle and
    last, output regions in reverse order with odd gaps"""
    rng = np.random.default_rng(8000)
    b = Batch(bw, bo)
    for i in range(15):
        b.lead((5 * i) % 16)
        if i in (4, 9, 14):
            b.seg()
        else:
            b.seg(*[fr(rng, int(rng.integers(0, 90)), b0=int(rng.choice([0x00, 0x80, 0x02, 0x89])), masked=bool(j % 3))
                    for j in range(int(rng.integers(1, 7)))], open_in=i % 2, cached_in=(i % 2) * 9)
    full = [i for i in range(15) if i not in (4, 9, 14)]
    perm = [full[i] for i in rng.permutation(len(full))]
    perm = [4] + perm[:6] + [9] + perm[6:] + [14]
    return b.done(8, out="reverse", perm=perm)


def auto_corner(nseg, mf, plus, bw=0, bo=0):
    """the auto rule's corners: nseg one-frame segments 16 bytes apart, buflen = (nseg << 18) + plus
    passed explicitly (the segments lie at the buffer's start; the rest of it is zeros)"""
    rng = np.random.default_rng(9000)
    b = Batch(bw, bo)
    body = rng.integers(0, 256, (nseg, 8), dtype=np.uint8)
    for s in range(nseg):
        b.gap(2)
        b.seg(Frame(bytes([0x80 if s % 3 else 0x00, 8]) + body[s].tobytes(), 0x82, body[s]))
    return b.done(mf, buflen=(nseg << 18) + plus)


def catalogue():
    """[(id, builder, kwargs, max_frames values to run it with)]; the builder's own max_frames first"""
    out = [("windows:L%d" % L, windows, {"L": L}, [4]) for L in LS]
    out += [("copy_phases", copy_phases, {}, [21]), ("ctl_bodies", ctl_bodies, {}, [8])]
    out += [("round_edges:" + e, round_edges, {"event": e}, [64]) for e in ("fin", "refused", "outspace")]
    out += [("frame_counts", frame_counts, {}, [64] + [m for m in MFS_BOTH + MFS_THREE if m != 64]),
            ("carry_first", carry_first, {}, [8])]
    out += [("u32_cached:%d" % lim, u32_cached, {"limit": lim}, [4]) for lim in U32_LIMITS]
    out += [("layout", layout, {}, [8])]
    return out


# ---------------------------------------------------------------------------------- classifier

def _placed(d, res_s, sl):
    """how many of the segment's frames have their body placed, by the delivery rule's stops"""
    nb, q = 0, 0
    nf, st = int(res_s["n_frames"]), int(res_s["status"])
    for k in range(nf):
        if int(d[k]["ret"]) <= 0 or int(d[k]["datalen"]) > sl - q or (st == -4 and k == nf - 1):
            break
        q += int(d[k]["datalen"])
        nb += 1
    return nb


def _windows(wb, lead, X, ends, nb, stop_x, stop_anywhere):
    """the fused kernel's windows of one segment: [(W0, W1, rule that chose the next window)] and
    the window index of every parsed header"""
    wins, where, i, w0, lend = [], [], 0, 0, 0
    while True:
        w1 = w0 + wb
        while i < len(X) and X[i] < w1:
            if i < nb:
                lend = ends[i]
            where.append(len(wins))
            i += 1
        ended = i == len(X) and (stop_anywhere or stop_x < w1)
        if lend > w1:
            wins.append((w0, w1, "body_pending"))
            w0 = w1
        elif not ended:
            nx = X[i] if i < len(X) else stop_x
            wins.append((w0, w1, "header:ph%d" % (nx & 15)))
            w0 = nx & ~15
        else:
            wins.append((w0, w1, "done"))
            return wins, where


def _fused_rounds(rets):
    """(round, lane) of every frame in the fused walk of a one-window segment"""
    out, i, r = [], 0, 0
    while i < len(rets):
        j = 0
        while i + j < len(rets) and j < 64 and rets[i + j] == rets[i]:
            j += 1
        lanes = j + 1 if j < 64 and i + j < len(rets) else j
        out += [(r, l) for l in range(lanes)]
        i += lanes
        r += 1
    return out


def features(case, L=None, mf=None, base=(0, 0)):
    """the cells a case reaches at window length L (default: every L of the kernel), max_frames mf
    (default: the case's own) and buffer base phases base = (wire, output)"""
    out = set()
    for l in ([L] if L else LS):
        out |= _features(case, l, mf or case[3], base)
    return out


def _features(case, L, mf, base):
    wire, so, sl, _, kw = case
    bw, bo = base
    flags = kw["flags"]
    od, orr, oms, oreg, oop, oca = oracle(case, mf)
    out, wb, G = set(), (L - 1) * 1024, RLAY_G
    if "buflen" in kw:
        out.add("auto:nseg%d:mf%d:buflen+%d" % (len(so), mf, kw["buflen"] - (len(so) << 18)))
    n = len(so)
    if any(so[i] > so[i + 1] for i in range(n - 1)):
        out.add("layout:permuted")
    if n > 2 and (sl[0] == 0, sl[n - 1] == 0) == (True, True) and any(x == 0 for x in sl[1:-1]):
        out |= {"layout:empty:first", "layout:empty:middle", "layout:empty:last"}
    oo = kw["out_off"]
    if n > 1 and all(oo[i] > oo[i + 1] + sl[i + 1] and (oo[i] - oo[i + 1] - sl[i + 1]) % 2 for i in range(n - 1)):
        out.add("layout:out_reverse_odd")
    for s in range(n):
        nf, st = int(orr[s]["n_frames"]), int(orr[s]["status"])
        d = od[s * mf:s * mf + nf]
        seglen, ob = int(sl[s]), int(oo[s])
        opened, cin = int(kw["open_in"][s]), int(kw["cached_in"][s])
        carry = opened == 1 and cin > 0
        cs = ":carry" if carry else ""
        lead = (bw + int(so[s])) & 15
        nb = _placed(d, orr[s], seglen)
        out.add("frames:%d:mf%d" % (nf, mf))
        if st == 1:
            out.add("stop:max_frames:mf%d" % mf)
        ok = [k for k in range(nf) if int(d[k]["ret"]) > 0]
        X = [int(d[k]["frame_off"]) - int(so[s]) + lead for k in ok]
        hl = [int(d[k]["hdrlen"]) for k in ok]
        pl = [int(d[k]["datalen"]) for k in ok]
        typ = [int(d[k]["type"]) for k in ok]
        ends = [X[k] + hl[k] + pl[k] for k in range(len(ok))]
        # where the walk stops (a refused frame is parsed, not consumed: consumed = its offset)
        stop_x = int(orr[s]["consumed"]) + lead
        wins, where = _windows(wb, lead, X, ends, nb, stop_x, st == 1 or int(orr[s]["consumed"]) >= seglen)
        if len(wins) > 1:
            out.add("L%d:lead%d" % (L, lead))
        for w, (w0, w1, rule) in enumerate(wins):
            if rule != "done":
                out.add("L%d:next:%s" % (L, rule))
            if w > 2:
                continue
            for k in range(len(ok)):
                pre = "L%d:w%d:" % (L, w)
                body = k < nb and pl[k] > 0
                if k < len(where) and where[k] == w and X[k] < w1 < X[k] + hl[k]:
                    out.add(pre + "hdr%d_split%d" % (hl[k], w1 - X[k]))
                if k < len(where) and where[k] == w + 1 and X[k] == w1:
                    out.add(pre + "hdr_at_edge:hdr%d" % hl[k])
                if body and X[k] + hl[k] == w1:
                    out.add(pre + "payload_at_edge:hdr%d" % hl[k])
                if ends[k] == w1:
                    out.add(pre + "frame_end_at_edge")
                if body and ends[k] - w1 in EDGE_D and X[k] + hl[k] < w1:
                    out.add(pre + "body_ends_past:%d" % (ends[k] - w1))
                if body and w1 - (X[k] + hl[k]) in EDGE_D and ends[k] > w1:
                    out.add(pre + "body_starts_before:%d" % (w1 - X[k] - hl[k]))
        edges = [w1 for (_, w1, _) in wins]
        for k in range(min(nb, len(ok))):
            c = sum(1 for e in edges if X[k] + hl[k] < e < ends[k])
            if c:
                out.add("L%d:body_crosses:%s" % (L, "3+" if c >= 3 else c))
        # copy phases and control bodies
        q = qc = 0
        for k in range(min(nb, len(ok))):
            isctl = bool(flags) and typ[k] & 8
            sp = (X[k] + hl[k]) & 15
            if isctl:
                qc += pl[k]
                dp = (bo + ob + seglen - qc) & 15
                out.add("ctl:zero_len" if pl[k] == 0 else "ctl:dst_ph%d" % dp)
            else:
                dp = (bo + ob + q) & 15
                q += pl[k]
            if pl[k] in COPY_LENS:
                out.add("copy:%s:%d:s%d:d%d" % ("m" if int(d[ok[k]]["masked"]) else "u", pl[k], sp, dp))
        if flags:
            data = [k for k in range(nb) if not typ[k] & 8]
            if nb and typ[0] & 8 and data:
                out.add("ctl:first")
            if nb and nb == nf and typ[nb - 1] & 8 and data and int(orr[s]["consumed"]) == seglen:
                out.add("ctl:last")
            frag = 0                                         # fragments of the open message so far
            for k in range(nb):
                if typ[k] & 8:
                    if frag and any(not typ[j] & 8 for j in range(k + 1, nb)):
                        out.add("ctl:between:%d" % (frag - 1))
                elif int(d[k]["is_fin"]):
                    frag = 0
                else:
                    frag += 1
            if st == 1 and nb == nf and typ[nf - 1] & 8:
                out.add("ctl:last_taken_at_max_frames")
            if st == -3 and nb < len(ok) and typ[nb] & 8:
                out.add("ctl:outspace")
            if opened and nf and typ[0] & 8:
                out.add("carry:first_ctl")
        if opened and nf and not (flags and typ[0] & 8):
            out.add("carry:first_fin" if int(d[0]["is_fin"]) else "carry:first_nonfin")
        if opened and nf == 0:
            out.add("carry:empty" if seglen == 0 else "carry:incomplete_hdr")
        if opened and cin in U32_CACHED and nf:
            lim = kw["readcache_max"]
            if st == -4 and nf == 1:
                out.add("u32:limit%d:cached%d:len%d:refused" % (lim, cin, pl[0]))
            elif nb:
                out.add("u32:limit%d:cached%d:len%d:taken" % (lim, cin, pl[0]))
                if cin + pl[0] >= 1 << 32:
                    out.add("u32:wrapped")
        # round edges (plain rule, one window, every frame of the run parsed)
        if not flags and len(wins) == 1 and len(ok) == nf:
            fus = _fused_rounds([int(d[k]["ret"]) for k in ok])
            events = []
            for (_, _, first, cnt, complete, cont) in oms[s]:
                if complete and (cnt > 1 or cont):
                    events.append(("fin_span", first + cnt - 1, first, bool(cont)))
            if st == -4:
                events.append(("refused", nf - 1, None, False))
            if st == -3:
                events.append(("outspace", nb, None, False))
            for ev, f, first, cont in events:
                if f >= len(fus):
                    continue
                sfx = cs
                if ev == "fin_span":
                    sfx = ":carry" if (cont and carry) else ""
                    if cont and not carry:
                        continue
                for impl, (r, l), last in (("lay", (f // G, f % G), G - 1), ("fus", fus[f], 63)):
                    if ev == "fin_span" and not cont:
                        r0 = first // G if impl == "lay" else fus[first][0]
                        if r0 == r:
                            continue                         # the message spans no round edge
                    if l in (0, last):
                        out.add("%s:%s:r%dl%d%s" % (impl, ev, min(r, 2), l, sfx))
    return out
