"""CPU checks of tests/dec_cases.py: the builders reach every kernel branch that
tests/test_gpu_decode_edges.py is meant to cover (REQUIRED, measured by dec_cases.features from
the oracle's output at the base shifts the GPU tests use), and the oracle restores the plaintext
the builders started from."""
import functools

import numpy as np
import pytest

import dec_cases as D
from oracle_lib import oracle_segments


def canon(p):
    """a pattern's wire lengths as letters (SAME: three headers, one wire length)"""
    return "A" * len(D.PATTERNS[p]) if p == "SAME" else D.PATTERNS[p]


PIECE_CELLS = (
    {"hdr%d_split%d" % (h, k) for h in D.HLS for k in range(1, h)}
    | {"payload_on_boundary:hdr%d" % h for h in D.HLS}
    | {"frame_end_on_boundary:hdr%d" % h for h in D.HLS}
    | {"piece_first_byte_in:" + w for w in ("gap", "tail", "header", "unmasked", "empty_seg", "payload")}
    | {"piece_gap:1", "piece_gap:17", "piece_gap:40"}
    | {"piece_tail:status-2", "piece_tail:status0", "piece_tail:status1"}
)
SMALL_CELLS = (
    {"small:%s:%d:ph%d" % (m, n, ph) for m in "mu" for n in D.SMALL_LENS for ph in range(16)}
    | {"seg_adjacent:gap0", "seg_adjacent:gap1"}
)
REQUIRED = (
    PIECE_CELLS | SMALL_CELLS
    | {"status:1", "status:0", "status:-2", "piece_first_byte_in:before_buf"}
    | {"wave_items:16", "wave_items:17", "wave_items:80", "wave_items:81", "wave_items:145+"}
    | {"ptr_delta:15", "ptr_delta:16", "ptr_delta:17", "wave_segments:17+"}
    | {"run:%d:%s" % (n, e) for n in D.RUN_N for e in D.RUN_ENDINGS}
    | {"run:%d:max_frames" % m for n in D.RUN_N for m in (n - 1, n) if m}
    | {"run:64:end", "run:64:max_frames"}
    | {"seq:period:AB", "seq:period:AABB", "seq:period:ABC", "seq:period:ABCD", "seq:period:ABCDE",
       "seq:period:AAAB", "seq:ABABAB8C", "same_len_diff_hdr"}
    | {"stop:%s:%s" % (kind, canon(p)[:k]) for p in D.PATTERNS for k in range(11) for kind in ("incomplete", "end")}
    | {"stop:max_frames:" + canon(p)[:m] for p in D.PATTERNS for m in D.ALPHA_MF if m < len(canon(p)) - 1}
    | {"long_not_first:AAA", "long_not_first:ABA", "long_not_first:ABAB"}
    | {"sf_hdr%d:%d" % (h, d) for h in D.HLS for d in D.SF_OFFSETS}
    | {"sf_straddle%d:%d" % (h, k) for h in D.HLS for k in range(1, h)}
    | {"sf_frame_end_at_W1", "sf_unmasked_jump"}
)
# Cells that cannot exist:
#  status:-1 (SEG_ERR_DECODE) needs a frame whose (int) length goes negative, >= 2^31 bytes
#    (tests/test_gpu_parity.py::test_int_truncation_real_size runs it at its real size);
#  a header of h bytes that starts k >= h bytes before a piece boundary or a window edge ends at or
#    before it, so it is not split (k == h is the cell payload_on_boundary).
IMPOSSIBLE = (
    {"status:-1"}
    | {"hdr%d_split%d" % (h, k) for h in D.HLS for k in list(range(h, 15)) + [0]}
    | {"sf_straddle%d:%d" % (h, k) for h in D.HLS for k in range(h, 15)}
)


@functools.lru_cache(maxsize=None)
def feats(cid, shift):
    (fn, kw, mfs), = [(f, k, m) for c, f, k, m in D.catalogue() if c == cid]
    case = fn(shift, **kw)
    out = set()
    for mf in mfs:
        out |= D.features(case[0], case[1], case[2], mf, shift)
    return frozenset(out)


IDS = [c[0] for c in D.catalogue()]


def test_required_cells_are_reached_and_impossible_ones_absent():
    got = set()
    for cid in IDS:
        for shift in D.shifts_of(cid):
            got |= feats(cid, shift)
    assert not REQUIRED - got, sorted(REQUIRED - got)[:20]
    assert not IMPOSSIBLE & got, sorted(IMPOSSIBLE & got)[:20]
    assert not REQUIRED & IMPOSSIBLE


@pytest.mark.parametrize("shift", range(16))
def test_geometric_cells_at_every_base_shift(shift):
    """the piece-boundary and chunk-phase cells hold at each base shift on its own: the builders
    place their frames in origin coordinates"""
    got = feats("piece_edges:short", shift) | feats("piece_edges:long", shift)
    assert not PIECE_CELLS - got, (shift, sorted(PIECE_CELLS - got))
    got = feats("small_payloads", shift)
    assert not SMALL_CELLS - got, (shift, sorted(SMALL_CELLS - got)[:10])
    if shift in (0, 1, 8, 15):
        got = feats("dense_items:frames", shift) | feats("dense_items:segments", shift)
        want = {c for c in REQUIRED if c.startswith(("wave_", "ptr_delta"))}
        assert not want - got, (shift, sorted(want - got))
        assert ("piece_first_byte_in:before_buf" in got) == (shift != 0)
        got = feats("segfuse_windows:edges", shift)
        want = {c for c in REQUIRED if c.startswith("sf_")}
        assert not want - got, (shift, sorted(want - got)[:10])


@pytest.mark.parametrize("cid", IDS)
def test_no_builder_is_feature_empty(cid):
    own = {"run_lengths": "run:", "alphabets": "stop:", "piece_edges": ("hdr", "piece_"), "small_payloads": "small:",
           "dense_items": ("wave_", "ptr_delta", "run:64:max_frames", "status:1"), "long_not_first": "long_not_first:",
           "segfuse_windows": ("sf_", "run:64:")}[cid.split(":")[0]]
    mine = {c for c in feats(cid, 0) & REQUIRED if c.startswith(own)}
    assert mine, cid


@pytest.mark.parametrize("cid", [c for c in IDS if not c.endswith(":sweep")])
def test_oracle_restores_the_builders_plaintext(cid):
    (fn, kw), = [(f, k) for c, f, k, m in D.catalogue() if c == cid]
    for shift in (0, 5):
        wire, so, sl, mf, plain = fn(shift, with_plain=True, **kw)
        if plain is None:                                      # a MAX_FRAMES stop leaves frames masked
            continue
        assert len(plain) == len(wire) and not np.array_equal(plain, wire)
        buf = wire.copy()
        desc, res = oracle_segments(buf, so, sl, mf)
        assert (res["status"] != 1).all()
        assert np.array_equal(buf, plain), (cid, int(np.nonzero(buf != plain)[0][0]))
        inside = np.zeros(len(wire), bool)
        for a, n in zip(so, sl):
            inside[a:a + n] = True
        assert (wire[~inside] == D.GAP).all() and (~inside).any()


def test_sweeps_cut_at_every_byte():
    for p in D.PATTERNS:
        wire, so, sl, mf = D.alphabets(0, p, "sweep")
        assert sl == list(range(len(sl))) and len(sl) - 1 <= D.SWEEP_BYTES
        whole = wire[so[-1]:so[-1] + sl[-1]]
        for i in (1, 7, len(sl) // 2):
            assert np.array_equal(wire[so[i]:so[i] + i], whole[:i])
        lens = D.sweep_frames(p)
        assert sum(lens) == sl[-1] and len(lens) >= 12
    assert set(D.sweep_frames("SAME")) == {106}


def test_case_sizes_and_segfuse_window():
    assert D.W1 == 17 * 1024
    for cid, fn, kw, mfs in D.catalogue():
        wire, so, sl, mf = fn(0, **kw)
        assert len(wire) <= 4 << 20, cid
        assert mf == mfs[0]
        assert all(a + n <= b for a, n, b in zip(so, sl, so[1:])), cid   # ascending, disjoint
    assert D.RUN_MF == [1, 2, 3, 14, 15, 16, 17, 18, 30, 31, 32, 33, 34, 47, 48, 49, 64]
