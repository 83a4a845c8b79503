"""tests/high_arena.py checked on the CPU: the byte-exact batch holds what it promises, every
listed placement puts the boundary on the feature it names, rebasing round-trips, and the low
alias windows never overlap the window they shadow."""
import numpy as np
import pytest

import dec_cases as D
import high_arena as H
from oracle_lib import oracle_segments


@pytest.fixture(scope="module")
def batch():
    wire, so, sl, mf, at = H.byte_exact()
    desc, res = oracle_segments(wire.copy(), so, sl, 8)       # all six frames of every segment
    return wire, so, sl, mf, at, desc, res


def frame_at(desc, res, x, mf=8):
    """(segment, index, descriptor) of the walked frame that holds wire offset x"""
    for s in range(len(res)):
        for j in range(int(res[s]["n_frames"])):
            d = desc[s * mf + j]
            if int(d["ret"]) > 0 and int(d["frame_off"]) <= x < int(d["frame_off"]) + int(d["ret"]):
                return s, j, d
    return None


def test_byte_exact_batch_holds_what_it_promises(batch):
    wire, so, sl, mf, at, desc, res = batch
    assert len(so) == 40 and mf == 4 and len(wire) < 4 << 20
    used = np.concatenate([desc[s * 8:s * 8 + int(res[s]["n_frames"])] for s in range(40)])
    used = used[used["ret"] > 0]
    assert set(int(x) for x in used["hdrlen"]) == set(D.HLS)
    for m in (0, 1):
        assert set(H.PAYLOADS) <= set(int(x) for x in used["datalen"][(used["masked"] != 0) == bool(m)])
    nf = [int(x) for x in res["n_frames"]]
    assert set(range(1, 7)) <= set(nf)
    assert int(res[39]["status"]) == -2                                       # ends in WRAP_HDR
    assert int(res[37]["status"]) == 0 and 0 < int(res[37]["consumed"]) < sl[37]       # truncated
    assert int(res[38]["status"]) == 0 and int(res[38]["consumed"]) == sl[38] - 5      # garbage tail
    d4, r4 = oracle_segments(wire.copy(), so, sl, mf)
    assert (r4["status"] == 1).any(), "max_frames 4 never stops a segment"
    assert (d4["data_off"] == np.uint64(H.DATA_OFF_NULL)).any() or (used["datalen"] == 0).any()


def test_every_at_hits_its_feature(batch):
    wire, so, sl, mf, at, desc, res = batch
    assert set(at) == {"hdr14:%d" % c for c in range(1, 14)} | {"payload_first", "payload_last", "payload_mid_chunk",
                                                                "frame_start", "segment_start", "gap"}
    for c in range(1, 14):
        s, j, d = frame_at(desc, res, at["hdr14:%d" % c])
        assert int(d["hdrlen"]) == 14 and at["hdr14:%d" % c] - int(d["frame_off"]) == c and j < mf
        assert frame_at(desc, res, at["hdr14:%d" % c] - 1)[2]["frame_off"] == d["frame_off"]
    s, j, d = frame_at(desc, res, at["payload_first"])
    assert at["payload_first"] == int(d["data_off"]) and int(d["masked"]) and j < mf
    assert at["payload_last"] == int(d["data_off"]) + int(d["datalen"]) - 1
    x = at["payload_mid_chunk"]
    assert int(d["data_off"]) + 16 < x < int(d["data_off"]) + int(d["datalen"]) - 16 and x % 16 == 7
    s, j, d = frame_at(desc, res, at["frame_start"])
    assert at["frame_start"] == int(d["frame_off"]) and 0 < j < mf
    assert at["segment_start"] in so and frame_at(desc, res, at["segment_start"])[1] == 0
    g = at["gap"]
    assert wire[g] == D.GAP and not any(a <= g < a + n for a, n in zip(so, sl))
    assert any(a + n <= g for a, n in zip(so, sl)) and any(a > g for a in so)
    assert len(H.header_ats(at)) == 14


def test_rebase_round_trips(batch):
    wire, so, sl, mf, at, desc, res = batch
    null = desc["data_off"] == np.uint64(H.DATA_OFF_NULL)
    for high in (H.place(H.B31, 77), H.place(H.B32, at["gap"]), H.ABOVE, H.place(H.B33, 1)):
        up = H.rebase(desc, high)
        assert np.array_equal(H.unrebase(up, high), desc)
        assert (up["frame_off"] == desc["frame_off"] + np.uint64(high)).all()
        assert (up["data_off"][null] == np.uint64(H.DATA_OFF_NULL)).all()
        assert (up["data_off"][~null] == desc["data_off"][~null] + np.uint64(high)).all()
        for f in ("datalen", "ret", "is_fin", "type", "masked", "hdrlen"):
            assert np.array_equal(up[f], desc[f])


def test_alias_windows_shadow_the_window_and_nothing_of_it(batch):
    wire, so, sl, mf, at, desc, res = batch
    n = len(wire)
    highs = [H.place(b, a) for b in H.BOUNDARIES.values() for a in at.values()]
    highs += [H.ABOVE, H.place_pieces(H.B32, 5 * D.PIECE + 3), H.place_pieces(H.ABOVE, 0), H.B32, H.B31, H.B33]
    for high in highs:
        lo, hi = H.window(high, n)
        assert 0 <= lo and hi <= H.ARENA_BYTES
        al = H.alias_windows(high, n)
        for (a, b), (c, d) in zip(al, al[1:]):
            assert b < c
        for a, b in al:
            assert 0 <= a < b and (b <= lo or a >= hi), (high, a, b)
        # every address of the window cut to 31 or 32 bits is the window's own or a sentinel's
        for x in (lo, high, high + 1, high + n // 2, high + n - 1, hi - 1) + tuple(b for b in (H.B31, H.B32, H.B33)
                                                                                  if lo <= b < hi):
            for m in H.MODULI:
                y = x % m
                assert lo <= y < hi or any(a <= y < b for a, b in al), (hex(high), hex(x), m)
        if high >= H.B31:
            assert al, hex(high)
    assert H.alias_windows(H.place(H.B31, n + H.GUARD), n) == []
    assert H.place(H.B32, 100) + 100 == H.B32 and H.place_pieces(H.B32, 3 * D.PIECE + 9) % D.PIECE == 0
    s = H.sentinel(5, 600)
    assert len(set(s.tolist())) > 200 and np.array_equal(s[10:20], H.sentinel(15, 25))
