"""CPU checks of tests/inflate_dev_cases.py: every hand-built token stream is accepted by the oracle
(CPython's zlib) and inflates to inflate_cases.played(ops), every body goes through the host rule
(websocketframeInflateHost) and equals the oracle there, and the builders hold the geometries that
tests/test_gpu_inflate_geometry.py relies on. No case is left out silently."""
import numpy as np

import inflate_cases as IC
import inflate_dev_cases as DV
import inflate_oracle as O
from util_amd import wsframe as W


def host_equals_oracle(body, tag):
    """the body through the host rule with room for exactly the oracle's output: (status, output)"""
    st, out = O.inflate_one(body)
    msg = np.array([(0, len(body), O.RAW, 0)], W.INFLATE_MSG_DTYPE)
    got, mr, res = W.inflate_host(np.frombuffer(body, np.uint8), msg, len(out))
    assert int(res["status"]) == st == int(mr[0]["status"]), "%s: host status %d, oracle %d" % (tag, int(res["status"]), st)
    assert got == out and int(mr[0]["out_len"]) == len(out), "%s: host output differs from the oracle's" % tag
    return st, out


def relation(dist, ln):
    return "<" if dist < ln else ("=" if dist == ln else ">")


def test_match_grid():
    grid = DV.match_grid()
    assert len(grid) == DV.GRID_COUNT
    assert {(p, d) for p, d, _, _, _ in grid} == {(p, d) for p in DV.GRID_P for d in DV.GRID_DIST if d <= p}
    for p, dist, ln, ops, body in grid:
        tag = "grid p %d dist %d len %d" % (p, dist, ln)
        st, out = host_equals_oracle(body, tag)
        assert st == O.OK and out == IC.played(ops), tag
        assert [(m[0], m[1], m[4]) for m in IC.fixed_block_matches(body)] == [(p, ln, dist), (p + ln + 3, 5, ln + 3)], tag
    # dist below, at and above len, each with the length (and the distance) on both sides of the 64 lanes
    assert {(relation(d, n), n > 64) for _, d, n, _, _ in grid if n != 64} == {(r, w) for r in "<=>" for w in (False, True)}
    assert {(relation(d, n), d > 64) for _, d, n, _, _ in grid if d != 64} == {(r, w) for r in "<=>" for w in (False, True)}
    # the run when the match arrives: empty (just flushed), one short of full, one past a flush
    assert {p % DV.RUN for p, _, _, _, _ in grid} >= {0, 1, 2, 63}
    assert sum(len(IC.played(ops)) for _, _, _, ops, _ in grid) < 1 << 20


def test_token_streams():
    streams = DV.token_streams()
    assert len(streams) == 500
    skip = fence_into_prev = skip_after_run = fence_after_run = full_runs = 0
    total = 0
    for k, (ops, body) in enumerate(streams):
        st, out = host_equals_oracle(body, "stream %d" % k)
        assert st == O.OK and out == IC.played(ops), k
        assert 3000 <= len(out) < 3300
        total += len(out)
        matches, runs = DV.io_trace(ops)
        full_runs += sum(n == DV.RUN for _, n in runs)
        for pos, dist, ln, run, fence, prev in matches:
            if prev is None:
                continue
            end = pos - dist + min(ln, dist)                  # one past the source's last byte
            if not fence and end <= prev[0]:
                skip += 1
                skip_after_run += run > 0
            if fence and end > prev[0] and pos - dist < prev[0] + prev[1]:
                fence_into_prev += 1
                fence_after_run += run > 0
    print("streams: %d bytes, skips %d (%d behind a run), fences into the previous match %d (%d behind a run), full runs %d"
          % (total, skip, skip_after_run, fence_into_prev, fence_after_run, full_runs))
    assert skip and fence_into_prev and skip_after_run and fence_after_run and full_runs
    used = [op for ops, _ in streams for op in ops if not isinstance(op, int)]
    assert {n for n, _ in used} == set(DV.STREAM_LENS)
    assert {d for _, d in used} >= {d for d in DV.STREAM_DISTS if d}


def test_io_trace_on_a_hand_made_list():
    ops = [1] * 64 + [2] * 3 + [(4, 2), (3, 60), 7, (5, 1), (3, 9)]
    matches, runs = DV.io_trace(ops)
    assert runs == [(0, 64), (64, 3), (74, 1)]
    # the first match waits (its source is the run before it), the second reads below that wait,
    # the third reads the literal before it, the fourth reads the second match's output: behind the wait
    assert matches == [(67, 2, 4, 3, True, None), (71, 60, 3, 0, False, (67, 4)), (75, 1, 5, 1, True, (71, 3)),
                       (80, 9, 3, 0, False, (75, 5))]
    assert len(IC.played(ops)) == 83


def test_stored_grid():
    grid = DV.stored_grid()
    assert [n for _, _, n in grid if n is not None] == list(DV.STORED_N) and set(DV.STORED_PAIRS) <= set(DV.STORED_N)
    verdicts, tails = set(), 0
    for name, body, n in grid:
        st, out = host_equals_oracle(body, name)
        if n is not None:
            assert st == O.OK and len(out) == n and bytes(body[DV.STORED_DATA_AT:DV.STORED_DATA_AT + n]) == out, name
        elif "+" in name:
            a, b = (int(v) for v in name.split()[1::2])
            assert st == O.OK and len(out) == a + b and out == body[5:5 + a] + body[10 + a:10 + a + b], name
        else:
            want, have = int(name.split()[2]), int(name.split()[4])
            verdicts.add(st)
            if st == O.OK and len(out) > have:
                tails += 1
                assert out == (b"xyz"[:have] + O.TAIL)[:len(out)] and len(out) == min(want, have + 4), name
    assert verdicts == {O.OK, O.ERR_DATA} and tails >= 3


def test_window_bodies():
    bodies = DV.window_bodies()
    names = [n for n, _ in bodies]
    assert len(names) == len(set(names))
    for kind, btype in (("dynamic", 2), ("fixed", 1), ("stored", 0)):
        mine = [b for n, b in bodies if n.startswith(kind)]
        assert all((b[0] >> 1) & 3 == btype and 250 <= len(b) <= 1600 for b in mine), kind
        assert {len(b) % 4 for b in mine} == {0, 1, 2, 3}, kind
        assert {DV.refills(b) for b in mine} >= set(range(1, 7)) if kind != "stored" else len(mine) >= 8, kind
    cuts = sorted(len(b) for n, b in bodies if n.startswith("prefix"))
    assert cuts == list(range(240, 281)) + list(range(500, 531))
    seen = set()
    for name, body in bodies:
        seen.add(host_equals_oracle(body, name)[0])
    assert seen == {O.OK, O.ERR_DATA} or seen == {O.OK}
