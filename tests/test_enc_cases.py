"""CPU checks of tests/enc_cases.py: encode_ref is pinned to oracle_encode_frames (the
oracle restatement of websocketframe.c:167-202 + RFC 6455 masking), and the builders hold
the geometries that tests/test_gpu_encode_edges.py relies on."""
import time

import numpy as np
import pytest

import enc_cases as E
from oracle_lib import oracle_encode_frames


def assert_ref_is_oracle(src, fr):
    want, woff = oracle_encode_frames(src, fr)
    got, off = E.encode_ref(src, fr)
    assert np.array_equal(off, woff)
    assert got.tobytes() == want


@pytest.mark.parametrize("seed", [1, 2])
def test_encode_ref_is_oracle_on_chain(seed):
    src, fr = E.chain(seed)
    assert 6000 <= len(fr) <= 10000
    assert_ref_is_oracle(src, fr)


def test_encode_ref_is_oracle_on_straddles():
    for lead0 in (0, 7):
        for case in E.STRADDLE_CASES:
            assert_ref_is_oracle(*E.straddle(*case, lead0=lead0))


@pytest.mark.parametrize("n", [n for n in E.COUNTS_N if n <= 513])
def test_encode_ref_is_oracle_on_counts(n):
    assert_ref_is_oracle(*E.counts(n))


def test_encode_ref_is_oracle_on_extended_type_and_flags():
    src, fr = E.flag_batch()
    assert len(fr) == 256 * 64
    seen = {(int(f["is_fin"]), int(f["prev_is_fin"]), int(f["masked"])) for f in fr[::256]}
    assert len(seen) == 64 and set(fr["type"][:256]) == set(range(256))
    assert_ref_is_oracle(src, fr)


def test_encode_ref_is_oracle_on_capacity_and_piece_batches():
    assert_ref_is_oracle(*E.capacity_batch())
    assert_ref_is_oracle(*E.capacity_batch_long())
    assert_ref_is_oracle(*E.capacity_boundary_batch(9))
    assert_ref_is_oracle(*E.per_piece(82))
    assert_ref_is_oracle(*E.per_wave(81, lead0=7))


def test_encode_ref_is_fast_enough():
    src, fr = E.counts(524289)
    t = time.perf_counter()
    wire, off = E.encode_ref(src, fr)
    dt = time.perf_counter() - t
    assert int(off[-1]) == len(wire)
    assert dt < 5.0, "encode_ref took %.2f s for 524289 tiny frames" % dt


def test_chain_draws():
    src, fr = E.chain(1)
    m = fr["masked"] != 0
    assert 0.6 < m.mean() < 0.85
    assert (fr["mask_key"][~m] != 0).mean() > 0.99                      # a key on unmasked frames too
    assert set(E.CHAIN_LENS) <= set(int(x) for x in fr["len"])
    assert set(fr["src_off"] & 15) == set(range(16))
    assert set(fr["type"]) == set(range(256))
    for name in ("is_fin", "prev_is_fin", "masked"):
        assert set(int(x) for x in fr[name]) == set(E.FLAGS), name
    so = fr["src_off"].astype(np.int64)
    assert (np.diff(so) < 0).mean() > 0.2                                # descending source offsets
    big = np.nonzero(fr["len"] >= 32)[0][:400]                           # payloads sharing source bytes
    a, b = so[big], so[big] + fr["len"][big].astype(np.int64)
    assert ((a[:, None] < b[None, :]) & (a[None, :] < b[:, None])).sum() > len(big)
    # a 64-bit length whose low two bytes are non-zero (65536 alone has them zero)
    assert ((fr["len"] > 65536) & ((fr["len"] & 0xFF) != 0) & (((fr["len"] >> 8) & 0xFF) != 0)).any()


def cells(*cols):
    return set(zip(*(c.tolist() for c in cols)))


@pytest.mark.parametrize("seed", [1, 2])
def test_chain_coverage(seed):
    """the three coverage conditions, at each of the 16 destination phases.

    Of the 768 cells d1 % 16 x next hl x next payload class x (own payload >= 32), 384 cannot
    exist: a 4/8- or 10/14-byte header is written only for payloads >= 126 bytes
    (websocketframe.c:167-174), so it never comes with payload class 0, 1-15 or 16-31. The
    other 384 must all occur, as must every one of the 96 and 256 cells of the other two."""
    src, fr = E.chain(seed)
    want1 = {(d, h, p, own) for d in range(16) for h in E.HLS for p in range(4) for own in (0, 1) if E.feasible(h, p)}
    assert len(want1) == 384
    assert {(h, p) for h in E.HLS for p in range(4) if not E.feasible(h, p)} == \
        {(h, p) for h in (4, 8, 10, 14) for p in (0, 1, 2)}
    want2 = {(o, h) for o in range(16) for h in E.HLS}
    want3 = {(s, d) for s in range(16) for d in range(16)}
    ln = fr["len"]
    nln = np.append(ln[1:], 0)
    for lead0 in range(16):
        c = E.classify(fr, lead0)
        has_next = c["nhl"] >= 0
        got1 = cells(c["d116"][has_next], c["nhl"][has_next], c["npc"][has_next], (c["pc"][has_next] == 3).astype(int))
        assert not want1 - got1, (lead0, sorted(want1 - got1)[:8])
        big = c["pc"] == 3
        got2 = cells(c["o16"][big], c["hl"][big])
        assert not want2 - got2, (lead0, sorted(want2 - got2))
        b48 = ln >= 48
        got3 = cells(c["s16"][b48], c["d016"][b48])
        assert not want3 - got3, (lead0, sorted(want3 - got3))
        # the two lengths just below the shift path's thresholds, at every phase: a 15-byte
        # payload after a >= 32-byte frame ending at d1 % 16, a 31-byte payload starting at o % 16
        n15 = has_next & (nln == 15) & big
        assert cells(c["d116"][n15], c["nhl"][n15]) == {(d, h) for d in range(16) for h in (2, 6)}, lead0
        l31 = ln == 31
        assert cells(c["o16"][l31], c["hl"][l31]) == {(o, h) for o in range(16) for h in (2, 6)}, lead0


def test_classify_on_a_hand_made_batch():
    fr = np.zeros(3, E.ENC_DTYPE)
    fr["len"] = [5, 126, 70000]
    fr["masked"] = [0, 1, 2]
    fr["src_off"] = [3, 16, 33]
    c = E.classify(fr, 5, capacity=150)
    assert c["o16"].tolist() == [5, 12, 2]                               # offsets 0, 7, 141
    assert c["hl"].tolist() == [2, 8, 14]
    assert c["pc"].tolist() == [1, 3, 3]
    assert c["d016"].tolist() == [7, 4, 0]
    assert c["d116"].tolist() == [12, 2, (5 + 141 + 14 + 70000) % 16]
    assert c["nhl"].tolist() == [8, 14, -1] and c["npc"].tolist() == [3, 3, -1]
    assert c["s16"].tolist() == [3, 0, 1]
    assert c["cut"].tolist() == [0, 0, 1]
    assert E.classify(fr, 0, capacity=7)["cut"].tolist() == [0, 2, 2]


def test_straddle_places_the_header():
    for lead0 in (0, 7):
        for (bd, hl, k) in E.STRADDLE_CASES:
            src, fr = E.straddle(bd, hl, k, lead0=lead0)
            _, off = E.encode_ref(src, fr)
            assert int(off[1]) + lead0 == bd - k
            c = E.classify(fr, lead0)
            assert int(c["hl"][1]) == hl and 0 < k < hl                  # the header crosses the boundary
            assert int(fr["len"][1]) >= 48 and int(fr["len"][2]) >= 48
    assert len(E.STRADDLE_CASES) == 3 * sum(h - 1 for h in E.HLS)


@pytest.mark.parametrize("lead0", [0, 7])
def test_per_piece_and_per_wave_counts(lead0):
    for m in E.PER_PIECE_M:
        src, fr = E.per_piece(m, lead0=lead0)
        _, off = E.encode_ref(src, fr)
        assert E.frames_touching(off, E.PIECE - lead0, 2 * E.PIECE - lead0) == m
        # the copy kernel's record loop sees frames [first, next piece's first]
        first, nxt = E.frame_at(off, E.PIECE - lead0), E.frame_at(off, 2 * E.PIECE - lead0)
        assert nxt - first + 1 == m
        src, fr = E.per_wave(m, lead0=lead0)
        _, off = E.encode_ref(src, fr)
        lo = E.PIECE + E.WAVE - lead0
        assert E.frames_touching(off, lo, lo + E.WAVE) == m
        assert E.frames_touching(off, E.PIECE - lead0, 2 * E.PIECE - lead0) == (m + 4 if m > 1 else 6)


def test_counts_tiles():
    tiles = [(n + E.TILE - 1) // E.TILE for n in E.COUNTS_N[-4:]]
    assert tiles == [1024, 1024, 1025, 2049]
    src, fr = E.counts(513)
    assert len(fr) == 513 and int(fr["len"].max()) <= 3


def test_capacity_batches():
    src, fr = E.capacity_batch()
    _, off = E.encode_ref(src, fr)
    assert 12 <= len(fr) <= 14 and 550 <= int(off[-1]) <= 800
    c = E.classify(fr, 0)
    assert set(c["hl"].tolist()) == {2, 4, 6, 8}
    assert {0, 5, 16, 31, 32, 40, 200} <= set(int(x) for x in fr["len"])
    for ln in (0, 5, 16, 32, 40):
        assert set((fr["masked"][fr["len"] == ln] != 0).tolist()) == {True, False}, ln
    src, fr = E.capacity_batch_long()
    assert {10, 14} <= set(E.classify(fr, 0)["hl"].tolist())
    for lead0 in (0, 1, 9, 15):
        src, fr = E.capacity_boundary_batch(lead0)
        _, off = E.encode_ref(src, fr)
        inside = (off[:-1].astype(np.int64) + lead0 > E.PIECE - 130) & (off[1:].astype(np.int64) + lead0 < E.PIECE + 400)
        assert inside.sum() >= 10                                        # the short frames lie around the boundary
        assert E.frames_touching(off, E.PIECE - lead0 - 40, E.PIECE - lead0 + 40) >= 3
