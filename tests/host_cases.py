"""The host-memory decode's planning (websocketframeBatchDecodeHost / ...HostMulti): an independent
model of its three rules and the directed batches that pin them.

Part 1 is the model, written from the comment blocks of include/wsframe_amd.h, ws_hostpath.hip and
ws_hostplan.h, in exact integer / Fraction arithmetic:
  groups   ordered segments (each starts at or after the end of the one before): a group takes the
           next segment while (that segment's end - the group's first offset) <= chunk and
           (segments * max_frames * 32) <= descriptor cap; it always holds its first segment. Any
           other layout: one group over all segments, lo / hi the min offset / max end.
  ranges   a group's non-empty segments in buffer order, touching or overlapping ones merged.
  cuts     nd = min(ndev, nseg) ranges; cut[r] is the segment boundary nearest to total * r / nd,
           the lower one on a tie, never below cut[r - 1]; of several boundaries at one byte
           position (empty segments) the last one when the position is at or below the share, the
           first one when above. ndev == 1, nseg < 2 or unordered segments: the one-device call.
Part 2 names the cells a layout reaches (from the model alone). Part 3 builds the directed layouts
and fills them with real frames. Part 4 places the geometric families of dec_cases.py at a host
offset. CPU only: numpy and dec_cases' frame builder.
"""
from fractions import Fraction

import numpy as np

import dec_cases as D

MIB = 1 << 20
DESC_BYTES = 32
DESC_CAP = 64 << 20
GAP = 0xA5

# ------------------------------------------------------------------------------------ 1. model


def inside(so, sl, buflen):
    return all(o <= buflen and l <= buflen - o for o, l in zip(so, sl))


def is_ordered(so, sl):
    return all(so[i] >= so[i - 1] + sl[i - 1] for i in range(1, len(so)))


def plan(so, sl, max_frames, buflen, chunk, cap=DESC_CAP):
    """None for a segment outside the buffer, else (ordered, [(s0, s1, lo, hi)])"""
    if not inside(so, sl, buflen):
        return None
    n = len(so)
    if n == 0:
        return True, []
    if not is_ordered(so, sl):
        return False, [(0, n, min(so), max(o + l for o, l in zip(so, sl)))]
    groups, s = [], 0
    while s < n:
        e = s + 1
        while e < n and so[e] + sl[e] - so[s] <= chunk and (e + 1 - s) * max_frames * DESC_BYTES <= cap:
            e += 1
        groups.append((s, e, so[s], so[e - 1] + sl[e - 1]))
        s = e
    return True, groups


def ranges(so, sl, group):
    s0, s1 = group[:2]
    out = []
    for a, b in sorted((so[s], so[s] + sl[s]) for s in range(s0, s1) if sl[s]):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(x) for x in out]


def single_device(so, sl, ndev):
    return ndev == 1 or len(so) < 2 or not is_ordered(so, sl)


def boundaries(sl):
    b = [0]
    for l in sl:
        b.append(b[-1] + l)
    return b


def cuts(sl, ndev):
    n = len(sl)
    nd = min(ndev, n)
    B = boundaries(sl)
    cut = [0] * (nd + 1)
    cut[nd] = n
    for r in range(1, nd):
        t = Fraction(B[-1] * r, nd)
        below = max(i for i in range(n + 1) if B[i] <= t)
        pick = below
        if below < n and B[below + 1] - t < t - B[below]:
            pick = below + 1
        cut[r] = max(pick, cut[r - 1])
    return cut


# ------------------------------------------------------------------------------------ 2. cells

PLAN_CELLS = [
    "close_by_bytes", "span_eq_chunk", "chunk_plus_1_breaks", "first_longer_than_chunk",
    "close_by_cap", "cap_exact_one_group", "cap_one_over",
    "zero_first_of_group", "zero_last_of_group", "zero_group_span0", "zero_at_buflen", "all_zero_call",
    "gap_1_in_group", "gap_4096_in_group", "gap_pushes_new_group", "merge_touching_next_to_gapped",
    "groups:1", "groups:2", "groups:3", "groups:4", "groups:7", "largest_group_last",
    "unordered", "outside", "nseg_0",
]
CUT_CELLS = [
    "ndev_gt_nseg", "single:ndev1", "single:nseg1", "single:unordered", "empty_range", "total_0", "exact_tie",
    "zero_len_at_cut", "weight_first", "weight_last",
]


def plan_cells(so, sl, max_frames, buflen, chunk, cap=DESC_CAP):
    p = plan(so, sl, max_frames, buflen, chunk, cap)
    if p is None:
        return {"outside"}
    ordered, groups = p
    n = len(so)
    if n == 0:
        return {"nseg_0"}
    out = {"groups:%d" % len(groups)}
    if not ordered:
        if len(ranges(so, sl, groups[0])) < sum(1 for l in sl if l):
            out.add("unordered")
        return out
    per = max_frames * DESC_BYTES
    spans = [hi - lo for _, _, lo, hi in groups]
    if max(spans) == 0:
        out.add("all_zero_call")
    if len(groups) >= 2 and all(spans[-1] > x for x in spans[:-1]):
        out.add("largest_group_last")
    for s in range(n):
        if sl[s] == 0 and so[s] == buflen:
            out.add("zero_at_buflen")
    for gi, (s0, s1, lo, hi) in enumerate(groups):
        k = s1 - s0
        if k == 1 and sl[s0] > chunk:
            out.add("first_longer_than_chunk")
        if k >= 2 and hi - lo == chunk:
            out.add("span_eq_chunk")
        if k >= 2 and sl[s0] == 0:
            out.add("zero_first_of_group")
        if k >= 2 and sl[s1 - 1] == 0:
            out.add("zero_last_of_group")
        if hi == lo:
            out.add("zero_group_span0")
        if k * per == cap and len(groups) == 1:
            out.add("cap_exact_one_group")
        for s in range(s0 + 1, s1):
            g = so[s] - (so[s - 1] + sl[s - 1])
            if g in (1, 4096):
                out.add("gap_%d_in_group" % g)
        r = ranges(so, sl, groups[gi])
        if 1 < len(r) < sum(1 for s in range(s0, s1) if sl[s]):
            out.add("merge_touching_next_to_gapped")
        if s1 < n:                                              # why the group closed before segment s1
            end = so[s1] + sl[s1]
            by_bytes, by_cap = end - lo > chunk, (k + 1) * per > cap
            if by_bytes and not by_cap:
                out.add("close_by_bytes")
                if end - lo == chunk + 1:
                    out.add("chunk_plus_1_breaks")
                if hi + sl[s1] - lo <= chunk:
                    out.add("gap_pushes_new_group")
            if by_cap and not by_bytes:
                out.add("close_by_cap")
                if k * per == cap and s1 + 1 == n:
                    out.add("cap_one_over")
    return out


def cut_cells(so, sl, ndev):
    n = len(so)
    out = set()
    if n == 0:
        return out
    if single_device(so, sl, ndev):
        if ndev == 1:
            out.add("single:ndev1")
        if n == 1:
            out.add("single:nseg1")
        if n >= 2 and ndev > 1:
            out.add("single:unordered")
        return out
    if ndev > n:
        out.add("ndev_gt_nseg")
    B = boundaries(sl)
    c = cuts(sl, ndev)
    nd = len(c) - 1
    if B[-1] == 0:
        out.add("total_0")
        return out
    if any(c[r] == c[r + 1] for r in range(nd)):
        out.add("empty_range")
    for r in range(1, nd):
        t = Fraction(B[-1] * r, nd)
        below = max(i for i in range(n + 1) if B[i] <= t)
        if below < n and B[below + 1] - t == t - B[below] and c[r] == below:
            out.add("exact_tie")
        if 0 < c[r] < n and (sl[c[r] - 1] == 0 or sl[c[r]] == 0):
            out.add("zero_len_at_cut")
    if sl[0] == B[-1]:
        out.add("weight_first")
    if sl[-1] == B[-1]:
        out.add("weight_last")
    return out


# ------------------------------------------------------------------------------------ 3. directed layouts

class Layout:
    """segments laid out left to right; gaps are 0xA5 bytes of the host buffer"""

    def __init__(self, name, max_frames=4, chunk=MIB, cap=DESC_CAP, gpu=True, ndevs=(), one_frame=False):
        self.name, self.max_frames, self.chunk, self.cap, self.gpu, self.ndevs = name, max_frames, chunk, cap, gpu, ndevs
        self.one_frame = one_frame                               # every segment a single frame
        self.so, self.sl, self.at, self.buflen = [], [], 0, None

    def gap(self, n):
        self.at += n
        return self

    def seg(self, *lens):
        for n in lens:
            self.so.append(self.at)
            self.sl.append(n)
            self.at += n
        return self

    def done(self, tail=0, buflen=None):
        self.buflen = self.at + tail if buflen is None else buflen
        return self

    def permuted(self, perm):
        self.so, self.sl = [self.so[i] for i in perm], [self.sl[i] for i in perm]
        return self

    def cells(self):
        return plan_cells(self.so, self.sl, self.max_frames, self.buflen, self.chunk, self.cap)


def _groups_n(n, C):
    """n groups: each opens with a segment of more than half a chunk (the next one cannot join) and
    takes a few small ones; the opening segments grow, so the largest group is the last"""
    L = Layout("groups_%d" % n, max_frames=3).gap(37)
    for i in range(n):
        L.seg((C * (55 + 5 * i)) // 100 + 13 * i)
        L.gap(i % 3).seg(700 + 11 * i, 300).gap(5 * (i % 2)).seg(1200)
    return L.done(tail=9)


def plan_layouts(C=MIB):
    """the directed group-plan layouts at chunk C (the GPU runs them at host_chunk_mb 1)"""
    out = [
        Layout("span_eq_chunk").gap(100).seg(C // 2, C // 2, 700).done(tail=3),
        Layout("chunk_plus_1").gap(5).seg(C // 2, C // 2 + 1, 300).done(tail=1),
        Layout("first_longer").gap(64).seg(C + 5, 300).gap(2).seg(200).done(tail=4),
        # 65536 frames of 32 descriptor bytes: 2 MiB per segment, 32 segments reach the 64 MiB cap
        Layout("cap_70_tiny", max_frames=65536).gap(3).seg(*([40] * 35)).gap(1).seg(*([23] * 35)).done(tail=2),
        # the cap as a parameter: 8 segments of 4 frames fill 1 KiB exactly; 9 are one over
        Layout("cap_exact_call", max_frames=4, cap=1024, gpu=False).seg(*([50] * 8)).done(),
        Layout("cap_one_over_call", max_frames=4, cap=1024, gpu=False).seg(*([50] * 9)).done(),
        # empty segments: first and last of a group; a group of its own (span 0) between a full group
        # and a segment longer than the chunk; one more at the very end of the buffer
        Layout("zero_positions").gap(50).seg(0, 300, C - 600, 0).seg(500, C - 500).gap(1).seg(0).seg(C + 1).seg(0).done(),
        Layout("all_zero", max_frames=2).gap(77).seg(0, 0, 0).done(tail=123),
        Layout("gaps_in_group").gap(9).seg(300).gap(1).seg(500).gap(4096).seg(700, 200, 100).gap(1).seg(50).done(tail=7),
        Layout("gap_pushes").gap(1).seg(C // 2).gap(C // 2).seg(300).done(tail=5),
    ]
    out += [_groups_n(n, C) for n in (1, 2, 3, 4, 7)]
    u = Layout("unordered").gap(11).seg(900, 300).gap(6).seg(450).gap(4096).seg(0, 120, 2000).gap(1).seg(77).done(tail=3)
    out.append(u.permuted([3, 0, 6, 1, 5, 2, 4]))
    out.append(Layout("outside").gap(8).seg(300, 200).done(buflen=8 + 300 + 199))
    out.append(Layout("nseg_0").gap(64).done())
    return out


def cut_layouts():
    """the directed multi-device layouts; each names the device counts it is made for (the GPU test
    runs every one of them on 2, 3 and 7 devices as well)"""
    def lay(name, lens, ndevs, gaps=(0, 3, 0, 1)):
        L = Layout(name, max_frames=3, ndevs=ndevs).gap(5)
        for i, n in enumerate(lens):
            L.seg(n).gap(gaps[i % len(gaps)])
        return L.done(tail=2)
    out = [
        lay("cut_ndev_gt_nseg", [400, 250, 900], (7,)),
        lay("cut_one_device", [300, 500, 200, 700], (1,)),
        lay("cut_one_segment", [800], (2, 3, 7)),
        lay("cut_giant", [200, 150, 600000, 300, 120, 90, 260, 410], (3, 7)),
        lay("cut_total_0", [0, 0, 0, 0], (2, 3, 7), gaps=(0, 2)),
        lay("cut_tie_2", [100, 200, 100], (2,)),
        lay("cut_tie_3", [200, 200, 500], (3,)),
        lay("cut_tie_7", [600, 200, 1000, 1000, 1000, 600, 500], (7,)),
        lay("cut_zero_below", [300, 0, 0, 301], (2,)),
        lay("cut_zero_at", [300, 0, 0, 300], (2,)),
        lay("cut_zero_above", [301, 0, 0, 300], (2,)),
        lay("cut_weight_first", [5000, 0, 0, 0], (2, 3, 7)),
        lay("cut_weight_last", [0, 0, 0, 5000], (2, 3, 7)),
    ]
    u = lay("cut_unordered", [300, 500, 200, 700], (2, 3, 7))
    out.append(u.permuted([2, 0, 3, 1]))
    return out


def growth_layouts(C=MIB):
    """slot growth across calls: a small call (three groups of a few KiB, far apart), one whose spans,
    segment counts and max_frames are all larger, and the small one again"""
    small = Layout("growth_small", max_frames=4).gap(19).seg(3000, 2000).gap(C).seg(4000).gap(2).seg(100).gap(C).seg(500)
    big = Layout("growth_big", max_frames=64).gap(7)
    for g in range(4):
        big.seg((C * (50 + 10 * g)) // 100)
        for i in range(40):
            big.gap(i % 2).seg(600 + 7 * i + g)
    return [small.done(tail=5), big.done(tail=1)]


def mixed_layouts(C=MIB):
    """one call whose groups take different decode paths under "path" -1 at max_frames 64: the largest
    span and the largest segment count over the groups fit the segment-fused path together, one
    group on its own does not. "tail": ~3500 one-frame segments of ~300 B fill the first group, ~900
    more are the tail group. "large_small": ~100 segments of ~10 KiB, then ~2000 of ~500 B"""
    rng = np.random.default_rng(77)
    tail = Layout("mixed_tail", max_frames=64, one_frame=True).gap(13)
    for i in range(4400):
        tail.seg(int(rng.integers(280, 321))).gap(int(rng.integers(0, 3)) if i % 5 == 0 else 0)
    ls = Layout("mixed_large_small", max_frames=64, one_frame=True).gap(29)
    for i in range(100):
        ls.seg(int(rng.integers(10000, 10400))).gap(i % 3)
    ls.gap(C // 16)
    for i in range(2000):
        ls.seg(int(rng.integers(480, 521))).gap(1 if i % 7 == 0 else 0)
    return [tail.done(tail=3), ls.done(tail=3)]


def prime_layout(C=MIB):
    """three groups of about one chunk, ten segments each (max_frames 4): every slot gets a small workspace"""
    L = Layout("mixed_prime", max_frames=4).gap(5)
    for g in range(3):
        for i in range(10):
            L.seg(C // 10 - 100 + i).gap(i % 2)
        L.gap(C // 8)
    return L.done(tail=2)


def model_groups(so, sl, max_frames, buflen, chunk, ndev=None):
    """the groups a host call launches: the whole call's, or with ndev those of each cut range"""
    if ndev is None or single_device(so, sl, ndev):
        return len(plan(so, sl, max_frames, buflen, chunk)[1])
    c = cuts(sl, ndev)
    return sum(len(plan(so[a:b], sl[a:b], max_frames, buflen, chunk)[1]) for a, b in zip(c, c[1:]))


def frame_exact(rng, total):
    """wire bytes of exactly `total`: one frame (a non-minimal length form where the minimal one
    cannot give the size, which the decode accepts); under 6 bytes an unmasked frame, 1 byte a cut header"""
    if total < 2:
        return bytes([0x82])[:total]
    if total < 6:
        return D.fr(rng, total - 2, masked=False)[0]
    if total - 6 < 126:
        return D.fr(rng, total - 6)[0]
    if total - 8 <= 0xFFFF:
        return D.fr(rng, total - 8, form=16)[0]
    return D.fr(rng, total - 14, form=64)[0]


def segment_bytes(rng, total):
    """a segment of exactly `total` bytes: one to three frames"""
    if total < 64:
        return frame_exact(rng, total)
    k = int(rng.integers(1, 4))
    cuts_ = sorted(int(x) for x in rng.integers(16, total - 16, k - 1)) if k > 1 else []
    parts = [b - a for a, b in zip([0] + cuts_, cuts_ + [total])]
    if min(parts) < 16:
        parts = [total]
    return b"".join(frame_exact(rng, p) for p in parts)


_filled = {}


def filled(layout):
    """the layout's host image: segments of real frames, every other byte 0xA5 (built once)"""
    if layout.name not in _filled:
        rng = np.random.default_rng(sum(layout.name.encode()))
        wire = np.full(layout.buflen, GAP, np.uint8)
        for o, n in zip(layout.so, layout.sl):
            if o + n <= layout.buflen:
                wire[o:o + n] = np.frombuffer((frame_exact if layout.one_frame else segment_bytes)(rng, n), dtype=np.uint8)
        _filled[layout.name] = wire
    return _filled[layout.name]


# ------------------------------------------------------------------------------------ 4. lo geometry
# A group's device buffer is a 256-B aligned slot holding the host bytes [lo, hi); the kernels get
# buf = slot - lo and the caller's offsets. Their origin coordinate of host byte x is x + (buf & 15)
# = x + (-lo mod 16): the group's first byte always sits at an origin that is a multiple of 16,
# whatever lo is, and 16 KiB pieces lie at multiples of 16384 of that coordinate. A dec_cases
# builder takes lead0 = the origin coordinate of its wire byte 0. With the wire at host offset
# `base` that is
#     lead0 = base + (-lo mod 16).
# Variant "open": the case's first segment opens the group, lo = base + seg_off[0], so lead0 +
# seg_off[0] must be the multiple of 16 at or above lo. Builders that open with a fixed gap solve
# that (lead0 = roundup16(lo) - gap); piece_edges places its first segment at an origin that is
# 5 mod 16 by construction and can never open a group at its own geometry: it runs in the second
# variant only. Variant "spacer": a segment of 1..15 bytes at host offset lo opens the group, a
# 0xA5 gap follows, then the wire: lead0 = base + (-lo mod 16) with no condition on the case, and
# every case byte's phase against the slot rotates with the spacer.

GEOM = [cid for cid in ("piece_edges:short", "piece_edges:long", "small_payloads", "dense_items:segments",
                        "long_not_first", "segfuse_windows:edges", "segfuse_windows:run64")]
GEOM_NO_OPEN = {"piece_edges:short", "piece_edges:long"}
LO_BASES = (20480 + 16, 4096 + 1, 32768 + 8, 12288 + 15)         # lo: each phase of {0, 1, 8, 15}, none a piece multiple
SPACERS = (1, 7, 15, 9)
SPACER_GAP = 21


def _builder(cid):
    for c, fn, kw, mfs in D.catalogue():
        if c == cid:
            return fn, kw, mfs[0]
    raise KeyError(cid)


def placed(cid, lo, variant):
    """(host image, seg_off, seg_len, max_frames, lead0) of the case in a group that starts at host
    offset lo; None when the variant cannot be built for it"""
    fn, kw, mf = _builder(cid)
    dev_lead = -lo % 16
    if variant == "open":
        lead0 = lo + dev_lead                                  # first try: a case whose first segment is at wire offset 0
        for _ in range(3):
            wire, so, sl, _mf = fn(lead0, **kw)
            if lead0 + so[0] == lo + dev_lead:
                break
            lead0 = lo + dev_lead - so[0]
        else:
            return None
        base = lo - so[0]
        if base < 0:
            return None
        head, extra_so, extra_sl = np.full(base, GAP, np.uint8), [], []
    else:
        n = SPACERS[LO_BASES.index(lo)]
        base = lo + n + SPACER_GAP
        lead0 = base + dev_lead
        wire, so, sl, _mf = fn(lead0, **kw)
        head = np.full(base, GAP, np.uint8)
        head[lo:lo + n] = np.frombuffer(frame_exact(np.random.default_rng(n), n), dtype=np.uint8)
        extra_so, extra_sl = [lo], [n]
    image = np.concatenate([head, wire, np.full(64, GAP, np.uint8)])
    return image, extra_so + [base + o for o in so], extra_sl + list(sl), mf, lead0
