"""CPU checks of tests/reasm_dir_cases.py: the builders reach every cell of the reassembly kernels
that tests/test_gpu_reasm_edges.py is meant to cover (REQUIRED, measured by
reasm_dir_cases.features from the oracle's output at the buffer base phases the GPU test uses), the
oracle's bodies are the plaintext the builders started from, and the oracle counts cached bytes in
u32 as the reference does."""
import functools

import numpy as np
import pytest

import reasm_dir_cases as D
from oracle_lib import cache_overflow
from reasm_ctl_oracle import region_image

G, TB = D.RLAY_G, D.RSEG_TB
EDGE_CELLS = (
    {"hdr%d_split%d" % (h, k) for h in D.HLS for k in range(1, h)}
    | {"hdr_at_edge:hdr%d" % h for h in D.HLS}
    | {"payload_at_edge:hdr%d" % h for h in D.HLS}
    | {"frame_end_at_edge"}
    | {"body_ends_past:%d" % d for d in D.EDGE_D}
    | {"body_starts_before:%d" % d for d in D.EDGE_D}
)
WINDOW_CELLS = (
    {"L%d:w%d:%s" % (L, w, c) for L in D.LS for w in (0, 1, 2) for c in EDGE_CELLS}
    | {"L%d:body_crosses:%s" % (L, c) for L in D.LS for c in ("1", "2", "3+")}
    | {"L%d:next:body_pending" % L for L in D.LS}
    | {"L%d:next:header:ph%d" % (L, p) for L in D.LS for p in range(16)}
    | {"L%d:lead%d" % (L, l) for L in D.LS for l in (0, 1, 15)}
)
COPY_CELLS = {"copy:%s:%d:s%d:d%d" % (m, n, s, d) for m in "mu" for n in D.COPY_LENS for s in range(16) for d in range(16)}
CTL_CELLS = (
    {"ctl:dst_ph%d" % p for p in range(16)}
    | {"ctl:zero_len", "ctl:first", "ctl:last", "ctl:between:0", "ctl:between:1", "ctl:between:2",
       "ctl:last_taken_at_max_frames", "ctl:outspace"}
)
ROUND_CELLS = (
    # the FIN frame that closes a message spanning a round edge: lane 0, the last lane, last + 1
    {"lay:fin_span:r1l0", "lay:fin_span:r1l%d" % (G - 1), "lay:fin_span:r2l0", "fus:fin_span:r1l0"}
    | {"lay:fin_span:r0l0:carry", "lay:fin_span:r0l%d:carry" % (G - 1), "lay:fin_span:r1l0:carry"}
    | {"fus:fin_span:r0l0:carry", "fus:fin_span:r0l%d:carry" % (TB - 1), "fus:fin_span:r1l0:carry"}
    | {"%s:%s:%s%s" % (impl, ev, pos, c) for ev in ("refused", "outspace") for c in ("", ":carry")
       for impl, pos in (("lay", "r0l0"), ("lay", "r0l%d" % (G - 1)), ("lay", "r1l0"),
                         ("fus", "r0l0"), ("fus", "r0l%d" % (TB - 1)), ("fus", "r1l0"))}
    | {"frames:%d:mf%d" % (n, TB) for n in (15, 16, 17, 63, 64)}
    | {"frames:65:mf65", "frames:65:mf200", "frames:200:mf200"}
    | {"stop:max_frames:mf%d" % m for m in D.MFS_BOTH + D.MFS_THREE}
)
CARRY_CELLS = (
    {"carry:first_fin", "carry:first_nonfin", "carry:first_ctl", "carry:empty", "carry:incomplete_hdr", "u32:wrapped"}
    | {"u32:limit%d:cached%d:len%d:%s" % (lim, c, n, "refused" if cache_overflow(c, n, lim) else "taken")
       for lim in D.U32_LIMITS for c in D.U32_CACHED for n in D.U32_LENS}
)
LAYOUT_CELLS = (
    {"layout:permuted", "layout:empty:first", "layout:empty:middle", "layout:empty:last", "layout:out_reverse_odd"}
    | {"auto:nseg%d:mf%d:buflen+%d" % c for c in D.AUTO_CORNERS}
)
REQUIRED = WINDOW_CELLS | COPY_CELLS | CTL_CELLS | ROUND_CELLS | CARRY_CELLS | LAYOUT_CELLS

# Cells that cannot exist:
#  a header of h bytes that starts k >= h bytes before a window edge ends at or before it, so it
#    is not split (k == h is the cell payload_at_edge);
#  without a message carried in, nothing spans a round edge before the second round, so no FIN
#    frame of round 0 closes such a message;
#  the fused kernel holds RSEG_TB = 64 frames per segment and one walk round takes up to 64, so a
#    second fused round is shorter than 64 frames (its last lane is never lane 63), and frame 64
#    ("last + 1" of a full round, fus:*:frame64) does not exist there: segments with more frames,
#    and max_frames above 64, run on the three-kernel path only; lane 0 of a later fused round is
#    reached after a frame of another wire length instead (fus:*:r1l0);
#  the u32 cells the other way round (a frame the reference's check_cache_overflow refuses cannot
#    be taken, and the reverse).
IMPOSSIBLE = (
    {"L%d:w%d:hdr%d_split%d" % (L, w, h, k) for L in D.LS for w in (0, 1, 2) for h in D.HLS for k in list(range(h, 15)) + [0]}
    | {"%s:fin_span:r0l%d" % (impl, l) for impl, l in (("lay", 0), ("lay", G - 1), ("fus", 0), ("fus", TB - 1))}
    | {"fus:%s:r1l%d%s" % (ev, TB - 1, c) for ev in ("fin_span", "refused", "outspace") for c in ("", ":carry")}
    | {"fus:%s:frame%d%s" % (ev, TB, c) for ev in ("fin_span", "refused", "outspace") for c in ("", ":carry")}
    | {"u32:limit%d:cached%d:len%d:%s" % (lim, c, n, "taken" if cache_overflow(c, n, lim) else "refused")
       for lim in D.U32_LIMITS for c in D.U32_CACHED for n in D.U32_LENS}
)

CATALOGUE = {cid: (fn, kw, mfs) for cid, fn, kw, mfs in D.catalogue()}
IDS = list(CATALOGUE)


@functools.lru_cache(maxsize=None)
def case(cid, base):
    fn, kw, _ = CATALOGUE[cid]
    return fn(bw=base[0], bo=base[1], **kw)


@functools.lru_cache(maxsize=None)
def feats(cid, base):
    out = set()
    for mf in CATALOGUE[cid][2]:
        out |= D.features(case(cid, base), mf=mf, base=base)
    return frozenset(out)


def auto_feats():
    out = set()
    for nseg, mf, plus in D.AUTO_CORNERS:
        out |= D.features(D.auto_corner(nseg, mf, plus), L=D.LS[0])
    return out


def test_required_cells_are_reached_and_impossible_ones_absent():
    got = auto_feats()
    for cid in IDS:
        for base in D.BASES:
            got |= feats(cid, base)
    print("REQUIRED cells: %d, reached: %d" % (len(REQUIRED), len(REQUIRED & got)))
    parts = (WINDOW_CELLS, COPY_CELLS, CTL_CELLS, ROUND_CELLS, CARRY_CELLS, LAYOUT_CELLS)
    assert len(REQUIRED) == sum(map(len, parts)) == 11553 and len(COPY_CELLS) == 2 * 21 * 256
    assert not REQUIRED - got, sorted(REQUIRED - got)[:20]
    assert not IMPOSSIBLE & got, sorted(IMPOSSIBLE & got)[:20]
    assert not REQUIRED & IMPOSSIBLE


@pytest.mark.parametrize("base", D.BASES)
def test_geometric_cells_at_each_base_phase(base):
    """the window-edge, copy-phase and control-body cells hold at each base phase on its own: the
    builders place their frames by address phase"""
    got = set()
    for cid in IDS:
        if cid.split(":")[0] in ("windows", "copy_phases", "ctl_bodies"):
            got |= feats(cid, base)
    want = WINDOW_CELLS | COPY_CELLS | CTL_CELLS
    assert not want - got, (base, sorted(want - got)[:20])


@pytest.mark.parametrize("cid", IDS)
def test_no_builder_is_feature_empty(cid):
    own = {"windows": "L", "copy_phases": "copy:", "ctl_bodies": "ctl:", "round_edges": ("lay:", "fus:"),
           "frame_counts": ("frames:", "stop:"), "carry_first": "carry:", "u32_cached": "u32:", "layout": "layout:"}
    mine = {c for c in feats(cid, D.BASES[0]) & REQUIRED if c.startswith(own[cid.split(":")[0]])}
    assert mine, cid


@pytest.mark.parametrize("cid", IDS)
def test_oracle_bodies_are_the_builders_plaintext(cid):
    """per segment: the bodies the oracle places are the plaintext of the segment's first frames, in
    order (data upward, control downward under CONTROL_DIRECT), and nothing else"""
    for base in D.BASES:
        c = case(cid, base)
        wire, so, sl, mf, kw = c
        inside = np.zeros(len(wire), bool)
        for a, n in zip(so, sl):
            inside[a:a + n] = True
        assert (wire[~inside] == D.GAP).all() and (~inside).any()
        for flags in (0, D.CTL):
            od, orr, oms, oreg, oop, oca = D.oracle(c, flags=flags)
            placed = 0
            for s in range(len(so)):
                data, ctl = [], []
                total = sum(len(b) for b in oreg[s][1:])
                for f in c.frames[s]:
                    if f.plain is None or sum(map(len, data + ctl)) + len(f.plain) > total:
                        break
                    (ctl if flags and f.b0 & 8 else data).append(f.plain)
                    placed += 1
                empty = np.zeros(0, np.uint8)
                assert np.array_equal(oreg[s][1], np.concatenate(data + [empty])), (cid, base, flags, s)
                if flags:
                    assert np.array_equal(oreg[s][2], np.concatenate(ctl[::-1] + [empty])), (cid, base, flags, s)
                    assert len(region_image(oreg[s], sl[s])) == sl[s]
            assert placed or cid.startswith("u32_cached"), cid


def test_carried_state_passes_segments_without_a_frame():
    """open_in 1 and an empty or incomplete-header segment: open state and cached bytes unchanged"""
    c = case("carry_first", D.BASES[0])
    for flags in (0, D.CTL):
        od, orr, oms, oreg, oop, oca = D.oracle(c, flags=flags)
        for s in range(len(c[1])):
            if int(orr[s]["n_frames"]) == 0:
                assert (int(oop[s]), int(oca[s]), oms[s]) == (1, c[4]["cached_in"][s], []), s
        assert sum(1 for s in range(len(c[1])) if int(orr[s]["n_frames"]) == 0) == 3


def _reference_u32(cached, frames, limit):
    """net_channel_ex.c:129-145 over u32 state, written from the reference's lines: cache_recv_bytes
    is `unsigned int` (transport_ctx.h), streamtransportctxCacheRecvPacket adds hdrlen (0 here) +
    bodylen to it (transport_ctx.c:182), the merge at a fragment_eof packet subtracts every merged
    packet's bytes again (transport_ctx.c:196): all modulo 2^32; check_cache_overflow
    (net_channel_ex.c:45-53) compares unsigned. frames: [(bodylen, fin)] with a message pending.
    Returns (frames taken, cache_recv_bytes at the end, detached)."""
    M = 1 << 32
    cached %= M
    mine = cached                                          # bytes of the packets in recvlist
    for i, (n, fin) in enumerate(frames):
        if limit > 0 and (limit < n or cached > limit - n):
            return i, cached, True
        cached = (cached + n) % M
        mine = (mine + n) % M
        if fin:
            cached = (cached - mine) % M
            mine = 0
    return len(frames), cached, False


@pytest.mark.parametrize("limit", D.U32_LIMITS)
def test_oracle_counts_cached_bytes_in_u32(limit):
    """cached_in 2^32 - 16 and 2^32 - 1, frames of 1..40 bytes, limit 0 and limits 1, 100, 2^32 - 1:
    oracle_reassemble stops, counts and wraps as the reference's u32 arithmetic does. The case rests
    on reading transport_ctx.c:179-201 and net_channel_ex.c:45-53, 129-145 (restated in
    _reference_u32): the reference reactor binary starts every connection at cache_recv_bytes = 0,
    so it reaches 2^32 - 16 only through a 4 GiB stream."""
    c = case("u32_cached:%d" % limit, D.BASES[0])
    wire, so, sl, mf, kw = c
    od, orr, oms, oreg, oop, oca = D.oracle(c)
    wrapped = 0
    for s in range(len(so)):
        frames = [(len(f.plain), f.b0 >> 7) for f in c.frames[s]]
        taken, cached, detached = _reference_u32(kw["cached_in"][s], frames, limit)
        st = int(orr[s]["status"])
        assert (st == -4) == detached, s
        assert int(orr[s]["n_frames"]) - (1 if detached else 0) == taken, s
        assert int(oca[s]) == (cached if int(oop[s]) else 0), s
        assert int(oop[s]) == (1 if detached else 0), s
        wrapped += kw["cached_in"][s] + frames[0][0] >= 1 << 32 and not detached
    assert (wrapped > 0) == (limit == 0)


def test_case_sizes_and_geometry():
    assert D.LS == (18, 20) and (G, TB) == (16, 64)
    for cid in IDS:
        wire, so, sl, mf, kw = case(cid, D.BASES[0])
        assert len(wire) <= 8 << 20 and max(sl) <= 80 << 10, cid
        assert mf == CATALOGUE[cid][2][0]
        regions = sorted(zip(kw["out_off"], sl))
        assert all(a + n <= b for (a, n), (b, _) in zip(regions, regions[1:])), cid
        assert regions[-1][0] + regions[-1][1] <= kw["out_size"], cid
