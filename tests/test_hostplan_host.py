"""The host-memory decode's plan (util_amd/csrc/ws_hostplan.h: groups, write-back ranges, multi-device
cuts), compiled for the host behind a thin C shim (tests/c/hostplan_host.cpp) and held against the
independent model of tests/host_cases.py: on every directed layout, and on a few thousand small
random ones with the chunk and the descriptor cap as free parameters, so every edge is cheap. The
invariants are checked on the header's own output by brute force; the directed set must reach
every cell of host_cases.PLAN_CELLS / CUT_CELLS. CPU only: g++, ctypes and numpy."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import host_cases as H

HERE = os.path.dirname(os.path.abspath(__file__))


class Plan:
    def __init__(self, lib):
        self.lib = lib
        vp, u64, u32, i32 = C.c_void_p, C.c_ulonglong, C.c_uint, C.c_int
        lib.ws_hostplan_groups.restype = C.c_longlong
        lib.ws_hostplan_groups.argtypes = [vp, vp, u32, u32, u64, u64, u64, vp, vp, vp, vp]
        lib.ws_hostplan_ranges.restype = u32
        lib.ws_hostplan_ranges.argtypes = [vp, vp, u32, u32, u64, u64, i32, vp]
        lib.ws_hostplan_cuts.restype = u32
        lib.ws_hostplan_cuts.argtypes = [vp, vp, u32, i32, vp]

    @staticmethod
    def _arrays(so, sl):
        return (np.ascontiguousarray(list(so) + [0], dtype=np.uint64), np.ascontiguousarray(list(sl) + [0], dtype=np.uint64))

    def groups(self, so, sl, max_frames, buflen, chunk, cap=None):
        """None (outside), else (ordered, groups, max_span, max_nseg); cap None: the header's default"""
        o, l = self._arrays(so, sl)
        g = np.zeros(4 * (len(so) + 1), dtype=np.uint64)
        ordered, span, mn = C.c_int(-1), C.c_ulonglong(0), C.c_uint(0)
        n = self.lib.ws_hostplan_groups(o.ctypes.data, l.ctypes.data, len(so), max_frames, buflen, chunk, cap or 0,
                                        g.ctypes.data, C.addressof(ordered), C.addressof(span), C.addressof(mn))
        if n < 0:
            return None
        return bool(ordered.value), [tuple(int(x) for x in g[4 * i:4 * i + 4]) for i in range(n)], span.value, mn.value

    def ranges(self, so, sl, group, ordered):
        o, l = self._arrays(so, sl)
        r = np.zeros(2 * (len(so) + 1), dtype=np.uint64)
        n = self.lib.ws_hostplan_ranges(o.ctypes.data, l.ctypes.data, group[0], group[1], group[2], group[3], int(ordered),
                                        r.ctypes.data)
        return [(int(r[2 * i]), int(r[2 * i + 1])) for i in range(n)]

    def cuts(self, so, sl, ndev):
        """None: the one-device call"""
        o, l = self._arrays(so, sl)
        c = np.zeros(len(so) + 2, dtype=np.uint32)
        nd = self.lib.ws_hostplan_cuts(o.ctypes.data, l.ctypes.data, len(so), ndev, c.ctypes.data)
        return None if nd == 0 else [int(x) for x in c[:nd + 1]]


@pytest.fixture(scope="module")
def hp(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("hostplan") / "libhostplan_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "c", "hostplan_host.cpp"),
                    "-o", so_path], check=True)
    return Plan(C.CDLL(so_path))


def check_plan(hp, so, sl, max_frames, buflen, chunk, cap, tag):
    """the header against the model, then the invariants on what the header gave"""
    got = hp.groups(so, sl, max_frames, buflen, chunk, cap)
    want = H.plan(so, sl, max_frames, buflen, chunk, H.DESC_CAP if cap is None else cap)
    if want is None:
        assert got is None, tag
        return
    assert got is not None, tag
    ordered, groups, max_span, max_nseg = got
    assert (ordered, groups) == want, (tag, got, want)
    n = len(so)
    capv = H.DESC_CAP if cap is None else cap
    assert [g[0] for g in groups] == [0] * bool(n) + [g[1] for g in groups[:-1]], tag      # a partition, in order
    assert (groups[-1][1] if groups else 0) == n and all(s0 < s1 for s0, s1, _, _ in groups), tag
    assert max_span == max([hi - lo for _, _, lo, hi in groups], default=0), tag
    assert max_nseg == max([s1 - s0 for s0, s1, _, _ in groups], default=0), tag
    brute = buflen <= 1 << 22                                   # byte maps of the whole buffer
    covered, back = np.zeros(buflen if brute else 0, bool), np.zeros(buflen if brute else 0, bool)
    for s in range(n if brute else 0):
        covered[so[s]:so[s] + sl[s]] = True
    for g in groups:
        s0, s1, lo, hi = g
        assert lo == min(so[s0:s1]) and hi == max(o + l for o, l in zip(so[s0:s1], sl[s0:s1])), tag
        if s1 - s0 > 1 and ordered:
            assert hi - lo <= chunk, (tag, g)
            assert (s1 - s0) * max_frames * H.DESC_BYTES <= capv, (tag, g)
        r = hp.ranges(so, sl, g, ordered)
        assert r == H.ranges(so, sl, g), (tag, g, r)
        assert all(a < b for a, b in r) and all(r[i][1] < r[i + 1][0] for i in range(len(r) - 1)), (tag, r)
        assert all(lo <= a and b <= hi for a, b in r), (tag, r)
        if brute:
            mine, got_bytes = np.zeros(buflen, bool), np.zeros(buflen, bool)
            for s in range(s0, s1):
                mine[so[s]:so[s] + sl[s]] = True
            for a, b in r:
                got_bytes[a:b] = True
            assert np.array_equal(got_bytes, mine), (tag, g)    # exactly the segments' bytes: no gap byte
            assert not (back & got_bytes).any(), (tag, g)       # no byte written back by two groups
            back |= got_bytes
    if brute:
        assert np.array_equal(back, covered), tag


def check_cuts(hp, so, sl, ndev, tag):
    got = hp.cuts(so, sl, ndev)
    if H.single_device(so, sl, ndev):
        assert got is None, (tag, got)
        return
    want = H.cuts(sl, ndev)
    assert got == want, (tag, got, want)
    n, nd = len(sl), min(ndev, len(sl))
    assert len(got) == nd + 1 and got[0] == 0 and got[nd] == n, tag
    assert all(got[r] <= got[r + 1] for r in range(nd)), tag
    B = H.boundaries(sl)
    for r in range(1, nd):
        t = Fraction(B[-1] * r, nd)
        best = min(abs(b - t) for b in B)
        if got[r] > got[r - 1]:                                 # not held up by the cut before it
            assert abs(B[got[r]] - t) == best, (tag, r, got)
        else:
            assert B[got[r]] >= t or abs(B[got[r]] - t) == best, (tag, r, got)


def test_directed_plan_layouts(hp):
    for L in H.plan_layouts():
        cap = None if L.cap == H.DESC_CAP else L.cap
        check_plan(hp, L.so, L.sl, L.max_frames, L.buflen, L.chunk, cap, L.name)
        # the same layout as the multi-device call's ranges see it
        for ndev in (1, 2, 3, 7):
            if H.inside(L.so, L.sl, L.buflen):
                check_cuts(hp, L.so, L.sl, ndev, L.name)


def test_directed_cut_layouts(hp):
    for L in H.cut_layouts():
        check_plan(hp, L.so, L.sl, L.max_frames, L.buflen, L.chunk, None, L.name)
        for ndev in (1, 2, 3, 7):
            check_cuts(hp, L.so, L.sl, ndev, "%s ndev %d" % (L.name, ndev))


def test_directed_set_reaches_every_cell():
    """from the model alone"""
    reached = set()
    for L in H.plan_layouts():
        reached |= L.cells()
    assert [c for c in H.PLAN_CELLS if c not in reached] == []
    reached = set()
    for L in H.cut_layouts():
        assert L.ndevs, L.name
        for ndev in L.ndevs:
            reached |= H.cut_cells(L.so, L.sl, ndev)
    assert [c for c in H.CUT_CELLS if c not in reached] == []
    for L in H.plan_layouts() + H.cut_layouts():               # segments never overlap: the oracle defines nothing there
        order = sorted(range(len(L.so)), key=lambda i: (L.so[i], L.sl[i]))
        assert all(L.so[b] >= L.so[a] + L.sl[a] for a, b in zip(order, order[1:])), L.name


def random_layout(rng):
    chunk = int(rng.choice([1, 2, 7, 64, 100, 4096, 5000]))
    nseg = int(rng.integers(1, 41))
    max_frames = int(rng.integers(1, 5))
    cap = int(rng.choice([0, 1, 3, 8, 40])) * max_frames * H.DESC_BYTES + int(rng.choice([0, 0, 1, 31]))
    so, sl, at = [], [], int(rng.choice([0, 0, 3, 4096]))
    for _ in range(nseg):
        n = int(rng.choice([0, 1, chunk - 1, chunk, chunk + 1, int(rng.integers(0, 3 * chunk + 2))]))
        so.append(at)
        sl.append(n)
        at += n + int(rng.choice([0, 0, 1, 4096, chunk + 1 + int(rng.integers(0, 50))]))
    buflen = max(o + l for o, l in zip(so, sl)) + int(rng.choice([0, 0, 5]))
    return so, sl, max_frames, buflen, chunk, max(cap, 1)


def test_random_layouts(hp):
    rng = np.random.default_rng(2024)
    seen = set()
    for it in range(3000):
        so, sl, mf, buflen, chunk, cap = random_layout(rng)
        kind = it % 8
        if kind == 5 and len(so) > 1:                           # out of buffer order (still no overlap)
            perm = rng.permutation(len(so))
            so, sl = [so[i] for i in perm], [sl[i] for i in perm]
        if kind == 6 and sl[-1]:
            buflen -= 1 + int(rng.integers(0, sl[-1]))          # the last segment pokes out of the buffer
        check_plan(hp, so, sl, mf, buflen, chunk, cap, "random %d" % it)
        seen |= H.plan_cells(so, sl, mf, buflen, chunk, cap)
        if H.inside(so, sl, buflen):
            for ndev in (1, 2, 3, 7) + ((5, 64) if it % 10 == 0 else ()):
                check_cuts(hp, so, sl, ndev, "random %d ndev %d" % (it, ndev))
    # the random layouts are no substitute for the directed ones, but they do meet the edges
    assert {"close_by_bytes", "close_by_cap", "span_eq_chunk", "chunk_plus_1_breaks", "first_longer_than_chunk",
            "zero_group_span0", "outside", "unordered"} <= seen


def test_default_cap_is_64_mib(hp):
    """the cap as the library runs it: 32 segments of 65536 frames, not 33"""
    for n, groups in ((32, 1), (33, 2)):
        so, sl = [10 * i for i in range(n)], [10] * n
        got = hp.groups(so, sl, 65536, 10 * n, 1 << 20)
        assert len(got[1]) == groups and got[1][0][1] == 32
