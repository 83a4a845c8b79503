"""The directed raw-stream cases of tests/stream_cases.py, checked on the CPU: every cell a builder
claims is true of the oracle's frame offsets under the model's geometry (tests/rwplan_model.py), every
splice leaves the length and the sample as they were, and the builders together reach every cell of
stream_cases.CELL_KINDS. No GPU."""
import numpy as np
import pytest

import rwplan_model as M
import stream_cases as S


def test_base_stream_geometry():
    wire, fo, fl = S.base_stream()
    g, P1, ch = S.base_chunks()
    assert len(wire) == S.BASE_BYTES and M.SAMPLE <= P1 < M.SAMPLE + 96
    P1b, nf, mean, smax = S.sample_of(fo, fl, len(wire))
    assert P1b == P1 and mean <= 64 and smax <= 96
    last = g.parts[g.nparts - 1]
    assert (last.P, last.C, last.H) == (P1, 65536, 8192) and 12 <= last.n <= 20
    # lengths change nearly every frame: the plan kernel's hint rule (fewer than 4 frames per header round)
    changes = int(np.count_nonzero(np.diff(fl[:nf]) != 0))
    assert changes * 4 > 3 * nf


@pytest.mark.parametrize("group", sorted(S.GROUPS))
def test_cells_hold_under_the_model(group):
    base, bfo, bfl = S.base_stream()
    _, P1, _ = S.base_chunks()
    for case in S.cases(group):
        fo, fl, res = S.frame_offsets(case.wire, case.max_frames)
        fo_all, fl_all, _ = S.frame_offsets(case.wire) if case.max_frames != S.BIG_MF else (fo, fl, res)
        geo = S.geometry(case.wire, opts=case.opts, fo=fo_all, fl=fl_all)
        assert geo is not None, case.name
        g, P1c, nf = geo
        # the sample is the base's: every byte before P1, and P1 itself
        if group != "aligned":                                    # (those have samples of their own, by design)
            assert P1c == P1 and np.array_equal(case.wire[:P1], base[:P1]), case.name
        if group not in ("stream_end",):
            assert len(case.wire) == len(base), case.name
        assert case.cells, case.name
        for cell in case.cells:
            S.check_cell(cell, case.wire, case.max_frames, g, fo_all, fl_all, res)


def test_every_cell_kind_is_reached_at_two_chunks():
    reached = {}
    for group in S.GROUPS:
        for case in S.cases(group):
            fo, fl, _ = S.frame_offsets(case.wire)
            g = S.geometry(case.wire, opts=case.opts, fo=fo, fl=fl)[0]
            nch = len(S.chunks_of(g))
            for cell in case.cells:
                k = S.cell_kind(cell, g)
                where = cell[1] if cell[0] in ("start", "hdr_cut", "zero_end", "entry", "long", "end", "next_hdr", "r2_jump", "pool") else case.name
                reached.setdefault(k, set()).add((where, nch))
    assert [k for k in S.CELL_KINDS if k not in reached] == []
    # each chunk-edge cell at two different chunk indices at the least, one of them the stream's last chunk
    for k, where in reached.items():
        if k.split()[0] in ("start", "hdr_cut", "zero_end", "entry", "end", "r2_jump", "pool") and not k.startswith("end part"):
            idx = {w for w, _ in where}
            assert len(idx) >= 2, (k, where)
            assert any(w == n - 1 for w, n in where), (k, where)
        if k.split()[0] == "next_hdr" or k == "long at window end":      # (need a next chunk: the last one that has one)
            assert len({w for w, _ in where}) >= 2 and any(w == n - 2 for w, n in where), (k, where)


def test_pass_loop_cases_are_what_they_claim():
    for name, wire, mf, opts, claim in S.pass_cases():
        fo, fl, res = S.frame_offsets(wire, mf)
        if claim[0] == "run":                                    # the leading run: exactly n equal frames, then another length
            n = claim[1]
            assert len(set(fl[:n])) == 1 and fl[n] != fl[0] and len(wire) < M.MIN_STREAM, name
        elif claim[0] == "changes":
            assert int(np.count_nonzero(np.diff(fl))) == claim[1] and len(wire) < M.MIN_STREAM, name
        elif claim[0] == "len":
            assert len(wire) == claim[1] and int(np.count_nonzero(np.diff(fl))) * 4 > 3 * len(fl), name
        else:
            assert int(res["n_frames"]) == claim[1], (name, res)
    for name, wire, mf, active in S.rest_cases():
        fo, fl, _ = S.frame_offsets(wire)
        P1, nf, mean, _ = S.sample_of(fo, fl, len(wire))
        assert M.short_rest(P1, len(wire), mean) == (not active) and len(wire) >= M.MIN_STREAM, name
    wire, n = S.pass_b_case()
    assert len(wire) == 6 * n and n > 8192 * 256 + 4096


def test_plan_stats_before_any_call():
    """a process that has made no chunk-planned call: every stream_plan_* stat is refused (-1)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from util_amd import wsframe as W\n"
            "for n in ('stream_plan_path', 'stream_plan_nchunks', 'stream_plan_P0', 'stream_plan_lk_walks2'):\n"
            "    try:\n        W.get_stat(n)\n    except ValueError:\n        continue\n    raise SystemExit(3)\n"
            "assert W.get_stat('stream_rw_chunks') == 0\n")
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0
