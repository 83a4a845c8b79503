"""Encode test cases: a vectorised reference encoder, deterministic case builders and a
geometry classifier for websocketframeBatchEncodeDevice (plain numpy, no torch).

encode_ref is written from the reference's rule (websocketframe.c:167-202: first byte from
(prev_is_fin, is_fin, type), 7/16/64-bit big-endian length) plus RFC 6455 §5.2-5.3 client
masking (MASK bit, the 4 key bytes, payload byte i XOR key byte i % 4). It is pinned to
oracle_encode_frames (the oracle restatement, itself pinned to the reference's golden
vectors) by tests/test_enc_cases.py and only then used as the expected output of the GPU
tests in tests/test_gpu_encode_edges.py.

classify models where each frame lies relative to the 16-byte output chunks. It only
measures what a batch covers; it never decides an expected byte.
"""
import functools

import numpy as np

from util_amd.wsframe import ENC_DTYPE

PIECE = 16384                       # one output piece (one block of the copy kernel)
WAVE = 4096                         # one wave's range inside a piece
TILE = 256                          # frames per tile of the front's scan
HLS = (2, 4, 6, 8, 10, 14)          # header lengths: 2 / 4 / 10, + 4 when masked
FLAGS = (0, 1, 2, 255)              # "false", "true" and two more non-zero bytes
CHAIN_LENS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 125, 126, 127, 300, 65535, 65536)
SRC_SLACK = 64


def head_len(n):
    """websocketframeEncodeHeadLength (websocketframe.c:167-174)"""
    return 2 if n < 126 else (4 if n <= 0xFFFF else 10)


def _geometry(frames):
    ln = frames["len"].astype(np.uint64)
    masked = frames["masked"] != 0
    base = np.where(ln < 126, 2, np.where(ln <= 0xFFFF, 4, 10)).astype(np.uint64)
    hl = base + np.where(masked, 4, 0).astype(np.uint64)
    offs = np.zeros(len(frames) + 1, np.uint64)
    np.cumsum(hl + ln, out=offs[1:])
    return ln, masked, base, hl, offs


def encode_ref(src, frames):
    """(wire uint8 array, offsets uint64[n + 1]) of the batch: every frame's header, key and
    (masked) payload back to back."""
    src = np.asarray(src, dtype=np.uint8)
    n = len(frames)
    ln, masked, base, hl, offs = _geometry(frames)
    wire = np.zeros(int(offs[-1]), np.uint8)
    o = offs[:-1].astype(np.int64)
    fin = frames["is_fin"] != 0
    pfin = frames["prev_is_fin"] != 0
    # websocketframe.c:178-189: type only when the previous frame was final, else CONTINUE (0)
    wire[o] = np.where(pfin, frames["type"], 0).astype(np.uint8) | np.where(fin, 0x80, 0).astype(np.uint8)
    b1 = np.where(base == 2, ln, np.where(base == 4, 126, 127)).astype(np.uint8)
    wire[o + 1] = b1 | np.where(masked, 0x80, 0).astype(np.uint8)
    m4 = base == 4
    for j in range(2):                                                   # memWriteBE16
        wire[o[m4] + 2 + j] = ((ln[m4] >> np.uint64(8 * (1 - j))) & np.uint64(0xFF)).astype(np.uint8)
    m10 = base == 10
    for j in range(8):                                                   # memWriteBE64
        wire[o[m10] + 2 + j] = ((ln[m10] >> np.uint64(8 * (7 - j))) & np.uint64(0xFF)).astype(np.uint8)
    key = frames["mask_key"].astype(np.uint32)
    ko = o[masked] + base[masked].astype(np.int64)
    for j in range(4):                                                   # key bytes in wire order
        wire[ko + j] = ((key[masked] >> np.uint32(8 * j)) & np.uint32(0xFF)).astype(np.uint8)
    d0 = o + hl.astype(np.int64)
    so = frames["src_off"].astype(np.int64)
    li = ln.astype(np.int64)
    long_ = li > 2048
    kb = np.zeros((n, 4), np.uint8)                                      # the XOR bytes (0 when unmasked)
    for j in range(4):
        kb[:, j] = np.where(masked, (key >> np.uint32(8 * j)) & np.uint32(0xFF), 0)
    for i in np.nonzero(long_)[0]:                                       # few long payloads: slices
        m = int(li[i])
        body = src[int(so[i]):int(so[i]) + m]
        assert len(body) == m, "payload outside src"
        wire[int(d0[i]):int(d0[i]) + m] = body ^ np.resize(kb[i], m)
    sh = np.nonzero(~long_ & (li > 0))[0]                                # many short ones: one gather
    if len(sh):
        cnt = li[sh]
        fid = np.repeat(sh, cnt)
        start = np.cumsum(cnt) - cnt
        pos = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(start, cnt)
        wire[d0[fid] + pos] = src[so[fid] + pos] ^ kb[fid, pos & 3]
    return wire, offs


CLASS_DTYPE = np.dtype([("o16", "i1"), ("hl", "i1"), ("pc", "i1"), ("d116", "i1"), ("nhl", "i1"), ("npc", "i1"),
                        ("s16", "i1"), ("d016", "i1"), ("cut", "i1")])


def pay_class(ln):
    """0: empty, 1: 1-15, 2: 16-31, 3: >= 32"""
    ln = np.asarray(ln, dtype=np.uint64)
    return np.where(ln == 0, 0, np.where(ln < 16, 1, np.where(ln < 32, 2, 3))).astype(np.int8)


def classify(frames, lead0, capacity=None):
    """per frame, with o = wire offset + lead0 (relative to the 16-byte aligned origin at or
    below dst), d0 = o + hl, d1 = d0 + len: o % 16, hl, payload class, d1 % 16, the next
    frame's hl and payload class (-1 for the last frame), src_off % 16, d0 % 16 and where the
    capacity cuts it (0: whole frame written, 1: cut inside, 2: nothing of it written)."""
    ln, masked, base, hl, offs = _geometry(frames)
    n = len(frames)
    o = offs[:-1] + np.uint64(lead0)
    d0 = o + hl
    d1 = d0 + ln
    c = np.zeros(n, CLASS_DTYPE)
    c["o16"] = o & np.uint64(15)
    c["hl"] = hl
    c["pc"] = pay_class(ln)
    c["d116"] = d1 & np.uint64(15)
    c["nhl"][:-1] = hl[1:]
    c["npc"][:-1] = c["pc"][1:]
    c["nhl"][-1:] = -1
    c["npc"][-1:] = -1
    c["s16"] = frames["src_off"] & np.uint64(15)
    c["d016"] = d0 & np.uint64(15)
    if capacity is not None:
        hi = np.uint64(lead0 + capacity)
        c["cut"] = np.where(d1 <= hi, 0, np.where(o >= hi, 2, 1))
    return c


def frame_at(offs, pos):
    """index of the frame whose wire extent holds byte `pos` (dst-relative)"""
    return int(np.searchsorted(offs, np.uint64(pos), side="right")) - 1


def frames_touching(offs, lo, hi):
    """number of frames with at least one wire byte in [lo, hi) (dst-relative); a frame always
    has >= 2 bytes"""
    a, b = offs[:-1].astype(np.int64), offs[1:].astype(np.int64)
    return int(np.count_nonzero((a < hi) & (b > lo)))


class _Batch:
    """frames appended back to back; payload sources drawn from one random src buffer"""

    def __init__(self, seed, src_len):
        self.rng = np.random.default_rng(seed)
        self.src = self.rng.integers(0, 256, src_len + SRC_SLACK, dtype=np.uint8)
        self.src_len = src_len
        self.rows = []
        self.cur = 0                                                     # wire offset of the next frame

    def add(self, ln, masked, src_phase=None, plain_flags=False):
        r = self.rng
        so = int(r.integers(0, self.src_len - ln + 1))
        if src_phase is not None:
            so = (so & ~15) + src_phase
            if so + ln > self.src_len:
                so -= 16 * ((so + ln - self.src_len + 15) // 16)
            assert so >= 0
        if plain_flags:
            row = (so, ln, int(r.integers(0, 2**32)), int(r.integers(0, 16)), int(r.integers(0, 2)),
                   int(r.integers(0, 2)), 1 if masked else 0)
        else:
            row = (so, ln, int(r.integers(0, 2**32)), int(r.integers(0, 256)), int(r.choice(FLAGS)),
                   int(r.choice(FLAGS)), int(r.choice(FLAGS[1:])) if masked else 0)
        self.rows.append(row)
        self.cur += head_len(ln) + (4 if masked else 0) + ln
        return len(self.rows) - 1

    def coin(self, p=0.75):
        return bool(self.rng.random() < p)

    def filler(self, wire_mod16):
        """one short frame of wire length = wire_mod16 (mod 16); none when that is 0 (half the time)"""
        if wire_mod16 % 16 == 0 and self.coin(0.5):
            return
        m = self.coin()
        h = 6 if m else 2
        ln = (wire_mod16 - h) % 16 + 16 * int(self.rng.integers(0, 3))
        self.add(ln, m)

    def done(self):
        fr = np.zeros(len(self.rows), ENC_DTYPE)
        for i, row in enumerate(self.rows):
            fr[i] = row
        return self.src, fr


def _lens_for(hl, pc):
    """payload lengths with header length hl (masked: 6, 8, 14) in payload class pc; empty
    where the header rule (websocketframe.c:167-174) allows none: a 4/10-byte length header
    means >= 126 bytes"""
    if hl in (2, 6):
        return {0: (0,), 1: (1, 2, 3, 15), 2: (16, 17, 31), 3: (32, 33, 47, 48, 49, 125)}[pc]
    if pc != 3:
        return ()
    return (126, 127, 300, 65535) if hl in (4, 8) else (65536, 70001)


def feasible(hl, pc):
    return len(_lens_for(hl, pc)) > 0


@functools.lru_cache(maxsize=None)
def chain(seed):
    """several thousand contiguous frames that hold, for every destination phase, every
    combination the edge logic distinguishes (tests/test_enc_cases.py checks the cells)"""
    b = _Batch(seed, 2 * 70001)
    own_big = (32, 33, 47, 48, 49, 125, 126, 127, 300)
    own_small = (0, 1, 2, 3, 15, 16, 17, 31)
    tick = 0
    # A: frame pairs — own payload (< 32 / >= 32) ending at every phase d1 % 16, followed by
    # every header length and payload class (every listed length of the class)
    for own in (own_small, own_big):
        for nhl in HLS:
            for npc in range(4):
                for nl in _lens_for(nhl, npc):
                    if nl == 65535 and own is own_small:
                        continue                                         # 300 B says the same; keeps the wire small
                    for t in range(16):
                        al = own[tick % len(own)]
                        am = b.coin()
                        tick += 1
                        b.filler(t - (b.cur + head_len(al) + (4 if am else 0) + al))
                        b.add(al, am)
                        assert b.cur % 16 == t
                        b.add(nl, nhl in (6, 8, 14))
    # B: every header length at every start phase o % 16 with a payload >= 32, and 31-byte
    # payloads (one below the shift path's threshold) likewise
    for hl in HLS:
        for ln in _lens_for(hl, 3)[-2:] + ((31,) if hl in (2, 6) else ()):
            for t in range(16):
                b.filler(t - b.cur)
                assert b.cur % 16 == t
                b.add(ln, hl in (6, 8, 14))
    # C: payloads >= 48 at every (source phase, payload start phase)
    big = (48, 49, 125, 126, 127, 300)
    for s in range(16):
        for t in range(16):
            ln = big[tick % len(big)]
            m = b.coin()
            tick += 1
            b.filler(t - (b.cur + head_len(ln) + (4 if m else 0)))
            b.add(ln, m, src_phase=s)
    # D: a random tail over the listed lengths (the 64 KiB ones rarely)
    w = np.array([0.002 if ln >= 65535 else 1.0 for ln in CHAIN_LENS])
    for ln in b.rng.choice(CHAIN_LENS, 2500, p=w / w.sum()):
        b.add(int(ln), b.coin())
        if b.coin(0.3):
            b.filler(int(b.rng.integers(0, 16)))
    return b.done()


def _len_with_hl(hl):
    """a payload >= 48 bytes whose (masked for 6, 8, 14) header is hl bytes; the 64-bit one
    has non-zero bytes in its low 16 bits"""
    return {2: 100, 6: 100, 4: 300, 8: 300, 10: 70001, 14: 70001}[hl]


STRADDLE_CASES = [(bd, hl, k) for bd in (PIECE, WAVE, 3 * WAVE) for hl in HLS for k in range(1, hl)]


def straddle(boundary, hl, k, lead0=0):
    """frame 1 has an hl-byte header that starts k bytes below `boundary` (relative to the
    aligned origin, i.e. at dst offset boundary - k - lead0), after one filler frame; a
    60-byte frame follows"""
    b = _Batch(boundary * 131 + hl * 17 + k, 70001 + 64)
    start = boundary - k - lead0
    b.add(start - 8, True)                                               # 126 <= len <= 65535: 8-byte header
    assert b.cur == start
    b.add(_len_with_hl(hl), hl in (6, 8, 14))
    b.add(60, b.coin())
    return b.done()


PER_PIECE_M = (1, 2, 15, 16, 17, 18, 64, 65, 80, 81, 82, 200, 1500)


def _tiny_run(b, count, room):
    """`count` frames of 0-3 payload bytes in at most `room` wire bytes"""
    if count <= 0:
        return
    avg = room / count
    assert avg >= 2
    for _ in range(count):
        if avg >= 9:
            b.add(int(b.rng.integers(0, 4)), b.coin())
        elif avg >= 3:
            b.add(int(b.rng.integers(0, 2)), False)
        else:
            b.add(0, False)


def per_piece(m, lead0=0):
    """exactly m frames touch piece 1 (origin-relative bytes [16384, 32768)): a large frame
    into it, m - 2 tiny frames, a large frame out of it (m = 1: one frame over all of it)"""
    b = _Batch(1000 + m, 40000)
    b.add(40, True)
    if m == 1:
        b.add(2 * PIECE + 500, b.coin())
        b.add(70, True)
        return b.done()
    b.add(PIECE + 100 - lead0 - b.cur - 8, True)                         # ends 100 bytes into piece 1
    assert b.cur + lead0 == PIECE + 100
    _tiny_run(b, m - 2, PIECE - 200)
    assert b.cur + lead0 < 2 * PIECE
    b.add(2 * PIECE + 300 - lead0 - b.cur, b.coin())                     # over the rest of piece 1
    b.add(70, True)
    return b.done()


def per_wave(m, lead0=0):
    """exactly m frames touch wave range 1 of piece 1 (origin-relative [20480, 24576)); three
    tiny frames and a medium one precede them in the piece, so the piece itself holds m + 4"""
    lo = PIECE + WAVE
    b = _Batch(2000 + m, 40000)
    b.add(40, True)
    b.add(PIECE + 100 - lead0 - b.cur - 8, True)
    _tiny_run(b, 3, 27)
    if m == 1:
        b.add(2 * WAVE + 77, b.coin())                                   # from wave range 0 over all of range 1
        b.add(3 * WAVE, True)
        return b.done()
    b.add(lo + 50 - lead0 - b.cur - 8, True)                             # ends 50 bytes into the range
    assert b.cur + lead0 == lo + 50
    _tiny_run(b, m - 2, WAVE - 100)
    assert b.cur + lead0 < lo + WAVE
    b.add(2 * PIECE + 300 - lead0 - b.cur, b.coin())
    b.add(70, True)
    return b.done()


COUNTS_N = (1, 2, 255, 256, 257, 511, 512, 513, 262143, 262144, 262145, 524289)


def counts(n):
    """n frames of 0-3 payload bytes (vectorised: the largest n is 2049 tiles of 256 frames)"""
    rng = np.random.default_rng(3000 + n)
    src = rng.integers(0, 256, 4096 + SRC_SLACK, dtype=np.uint8)
    fr = np.zeros(n, ENC_DTYPE)
    fr["len"] = rng.integers(0, 4, n)
    fr["src_off"] = rng.integers(0, 4090, n)
    fr["mask_key"] = rng.integers(0, 2**32, n, dtype=np.uint64)
    fr["type"] = rng.integers(0, 256, n)
    fr["is_fin"] = rng.choice(FLAGS, n)
    fr["prev_is_fin"] = rng.choice(FLAGS, n)
    fr["masked"] = np.where(rng.random(n) < 0.25, rng.choice(FLAGS[1:], n), 0)
    return src, fr


def capacity_batch():
    """12 frames, about 600 wire bytes: all six header lengths, payloads 0, 5, 16, 31, 32, 40
    and 200, masked and unmasked"""
    b = _Batch(4001, 4096)
    for ln, m in ((40, True), (0, False), (5, True), (16, False), (126, False), (31, True), (32, False),
                  (200, True), (0, True), (16, True), (130, True), (40, False), (5, False), (32, True)):
        b.add(ln, m)
    return b.done()


def capacity_batch_long():
    """the 10- and 14-byte headers need >= 64 KiB payloads, so they cannot sit in a 600-byte
    batch: here they are, between short frames; capacity_cuts_long lists the cuts around
    every frame's start, payload start and end"""
    b = _Batch(4002, 70001 + 64)
    for ln, m in ((40, True), (70001, False), (5, True), (31, False), (70001, True), (32, True), (16, False)):
        b.add(ln, m)
    return b.done()


def capacity_cuts_long(frames, margin=20):
    _ln, _m, _base, hl, offs = _geometry(frames)
    cuts = set()
    for i in range(len(frames)):
        for p in (int(offs[i]), int(offs[i] + hl[i]), int(offs[i + 1])):
            cuts.update(range(max(0, p - margin), p + margin + 1))
    return sorted(cuts)


def capacity_boundary_batch(lead0=0):
    """frames of 0-200 payload bytes laid over the first piece boundary (origin-relative 16384)"""
    b = _Batch(4100 + lead0, 20000)
    b.add(PIECE - 120 - lead0 - 8, True)
    for ln, m in ((40, False), (0, True), (31, True), (5, False), (32, True), (16, False), (16, True), (0, False),
                  (40, True), (200, False), (33, True)):
        b.add(ln, m)
    return b.done()


def flag_batch():
    """type 0..255 x (is_fin, prev_is_fin, masked) each in {0, 1, 2, 255}: one frame each"""
    rng = np.random.default_rng(5001)
    n = 256 * 64
    src = rng.integers(0, 256, 4096 + SRC_SLACK, dtype=np.uint8)
    fr = np.zeros(n, ENC_DTYPE)
    i = np.arange(n)
    fr["type"] = i & 255
    fr["is_fin"] = np.array(FLAGS)[(i >> 8) & 3]
    fr["prev_is_fin"] = np.array(FLAGS)[(i >> 10) & 3]
    fr["masked"] = np.array(FLAGS)[(i >> 12) & 3]
    fr["len"] = rng.integers(0, 41, n)
    fr["src_off"] = rng.integers(0, 4000, n)
    fr["mask_key"] = rng.integers(0, 2**32, n, dtype=np.uint64)
    return src, fr
