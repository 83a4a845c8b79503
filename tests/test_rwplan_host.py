"""The geometry of the raw stream's chunk-parallel walk (util_amd/csrc/ws_rwplan.h: chunk, window,
parts of a split walk, list sizes and bases; the host-linked walk's rule), compiled for the host
behind a thin C shim (tests/c/rwplan_host.cpp) and held against the independent exact-integer model
of tests/rwplan_model.py: on directed inputs at every edge of the rule and on a few thousand seeded
random ones. The invariants are checked on the header's own output. CPU only: g++, ctypes, numpy."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import rwplan_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
KIB = 1 << 10
BIG = 1 << 40                       # caps that never bind
NBIG = (1 << 32) - 1                # (the chunk cap is 32 bits)


class Shim:
    def __init__(self, lib):
        self.lib = lib
        u64, u32, vp = C.c_ulonglong, C.c_uint, C.c_void_p
        lib.ws_rwplan_device.restype = C.c_int
        lib.ws_rwplan_device.argtypes = [vp, vp]
        lib.ws_rwplan_hostgeo.restype = None
        lib.ws_rwplan_hostgeo.argtypes = [u64, u64, u64, u64, vp]
        lib.ws_rwplan_window.restype = u32
        lib.ws_rwplan_window.argtypes = [u64, u32, u64]
        lib.ws_rwplan_mean.restype = u64
        lib.ws_rwplan_mean.argtypes = [u64, u64, u64]
        lib.ws_rwplan_short_rest.restype = C.c_int
        lib.ws_rwplan_short_rest.argtypes = [u64, u64, u64]
        lib.ws_rwplan_consts.restype = None
        lib.ws_rwplan_consts.argtypes = [vp]

    def device(self, P1, length, mean, longest, cmin, cmax, ncap, ccap, scap, xs=(0, 0), shifts=(0, 0)):
        a = np.array([P1, length, mean, longest, cmin, cmax, ncap, ccap, scap, xs[0], xs[1], shifts[0], shifts[1]],
                     dtype=np.uint64)
        o = np.zeros(2 + 9 * M.NP, dtype=np.uint64)
        if self.lib.ws_rwplan_device(a.ctypes.data, o.ctypes.data) != 0:
            return None
        parts = [M.Part(*(int(v) for v in o[2 + 9 * k:11 + 9 * k])) for k in range(M.NP)]
        return M.Geom(parts, int(o[0]), int(o[1]))

    def host(self, P1, length, mean, cmax):
        o = np.zeros(5, dtype=np.uint64)
        self.lib.ws_rwplan_hostgeo(P1, length, mean, cmax, o.ctypes.data)
        return tuple(int(v) for v in o)


@pytest.fixture(scope="module")
def rp(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("rwplan") / "librwplan_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "c", "rwplan_host.cpp"),
                    "-o", so_path], check=True)
    return Shim(C.CDLL(so_path))


def check(rp, args, tag):
    """the header against the model, then the invariants on what the header gave"""
    P1, length, mean, longest, cmin, cmax, ncap, ccap, scap, xs, shifts = args
    got = rp.device(*args)
    assert got is not None, tag
    want = M.device_plan(*args)
    assert got == want, (tag, got, want)
    np_ = got.nparts
    assert 1 <= np_ <= M.NP, tag
    # the parts tile [P1, len): no gap, no overlap, chunk grids that end where the next begins
    at, cb, sb, db = P1, 0, 0, 0
    for k, t in enumerate(got.parts):
        assert (t.cbase, t.stg_base, t.cand_base) == (cb, sb, db), (tag, k)   # (an empty part's bases: the next part's)
        if k >= np_:
            assert t.n == 0 and t.P == length, (tag, k)
            continue
        assert t.P == at, (tag, k, t, at)
        last = k + 1 == np_
        end = length if last else min(length, t.P + t.n * t.C)
        assert t.n == M.ceil_div(end - t.P, t.C), (tag, k)
        if not last:
            assert end == length or end == t.P + t.n * t.C, (tag, k)          # a whole number of chunks
        at = end
        hi_c = max(cmin, cmax)
        assert t.C & (t.C - 1) == 0 and t.C >= M.CMIN, (tag, k, t.C)
        if ncap == NBIG and ccap >= BIG and scap >= BIG:
            assert t.C <= hi_c, (tag, k, t.C)                                 # (unless the caps forced it up)
        assert t.H % 4096 == 0 and M.HMIN <= t.H <= min(t.C // 2, M.HMAX), (tag, k, t.H)
        assert t.capc >= 64 and t.stgn >= 64, (tag, k)
        assert t.capc <= t.H // 32 and t.stgn <= M.STGN_DEV, (tag, k)
        cb, sb, db = cb + t.n, sb + t.n * M.OWNERS * t.stgn, db + t.n * t.capc
    assert at == length, tag
    assert got.nchunks == cb and cb <= ncap and sb <= scap and db <= ccap, (tag, cb, sb, db)
    # a cut inside the rest is a part's end rounded up to its chunk grid: never before the cut
    B = P1
    for k in range(np_ - 1):
        t = got.parts[k]
        end = min(length, t.P + t.n * t.C)
        assert end >= min(xs[k], length) or xs[k] <= B, (tag, k)
        assert end - max(xs[k], B) < t.C or xs[k] <= B, (tag, k)              # and less than a chunk past it
        B = end
    return got


def test_constants_are_the_models(rp):
    o = np.zeros(12, dtype=np.uint64)
    rp.lib.ws_rwplan_consts(o.ctypes.data)
    assert [int(v) for v in o] == [M.CMIN, M.CMAX, M.HMIN, M.HMAX, M.SAMPLE, M.MIN_STREAM, M.MIN_FRAMES, M.NP, M.OWNERS,
                                   M.STGN_DEV, M.STGN_HOST, M.CAP_CHUNKS]


MEANS = (1, 63, 64, 65, 4096)
SEENS = (0, 1, 4095, 4096, 128 * KIB - 4096, 128 * KIB - 4095)


def test_window_edges(rp):
    for mean, seen, c in itertools.product(MEANS + (0, 1023, 1024, 1025, 32 * KIB, 40000), SEENS + (4097, 8191, 8192, 1 << 20, 0xFFFFFFFF),
                                           [M.CMIN << k for k in range(9)]):
        h = rp.lib.ws_rwplan_window(mean, seen, c)
        assert h == M.window(mean, seen, c), (mean, seen, c)
        assert h % 4096 == 0 and 4096 <= h <= min(c // 2, 128 * KIB)
        if seen + 4096 <= min(c // 2, 128 * KIB):
            assert h > seen                                               # longer than every frame seen
    # the values the issue names: a 20 KiB frame gives a window of 24 KiB (at least: 4 KiB steps)
    assert rp.lib.ws_rwplan_window(60, 20 * KIB, 65536) == 24 * KIB
    assert rp.lib.ws_rwplan_window(60, 20 * KIB + 1, 65536) == 28 * KIB
    assert rp.lib.ws_rwplan_window(60, 90, 65536) == 8 * KIB              # 90 + 4096 rounded up
    assert rp.lib.ws_rwplan_window(60, 0, 65536) == 4 * KIB
    assert rp.lib.ws_rwplan_window(64, 128 * KIB - 4096, 1 << 20) == 128 * KIB
    assert rp.lib.ws_rwplan_window(64, 1 << 20, 65536) == 32 * KIB        # C / 2 binds


def test_mean_and_short_rest(rp):
    for P, P1, fr in ((0, 262170, 4100), (5, 5, 0), (0, 300000, 1), (7, 262151, 3), (0, 262144, 262144)):
        assert rp.lib.ws_rwplan_mean(P, P1, fr) == M.mean_of(P, P1, fr)
    for mean in (0, 1, 63, 64, 65, 4096):
        m = max(mean, 1)
        for rest in (255 * m - 1, 255 * m, 256 * m - 1, 256 * m, 256 * m + 1, 1):
            if rest > 0:
                got = rp.lib.ws_rwplan_short_rest(1000, 1000 + rest, mean)
                assert got == int(M.short_rest(1000, 1000 + rest, mean)) == int(rest // m < 256), (mean, rest)


def test_directed_plans(rp):
    P1 = 262200
    n = 0
    for mean, seen in itertools.product(MEANS, SEENS):
        C0 = M.pow2_from(1024 * mean, M.CMIN, 1 << 22)
        # lengths that end exactly on a chunk start, one byte before and after it, and one byte into the rest
        for length in (P1 + 20 * C0, P1 + 20 * C0 - 1, P1 + 20 * C0 + 1, P1 + 1, P1 + C0, P1 + 3 * C0 + 4097):
            # cuts at, before and after P1, past len, equal to each other, on a chunk start and one byte past it
            cuts = [(0, 0), (P1, 0), (P1 - 1, P1 + 1), (P1 + 1, 0), (P1 + C0, P1 + C0), (P1 + C0, P1 + C0 + 1),
                    (P1 + C0 + 1, P1 + 5 * C0), (P1 + 5 * C0, P1 + C0), (length, 0), (length - 1, length + 5),
                    (P1 + 2 * C0, length), (0, P1 + 2 * C0), (1, 2), (length + 1, P1 + 2)]
            for xs in cuts:
                for shifts in ((0, 0), (3, 2), (6, 6), (1, 5)):
                    check(rp, (P1, length, mean, seen, M.CMIN, 1 << 22, NBIG, BIG, BIG, xs, shifts), (mean, seen, length, xs, shifts))
                    n += 1
    assert n > 5000
    # every shift 0..6 for each of the two cuts, where the shift matters (chunks of 4 MiB) and where the
    # window's need clamps it (a window of 128 KiB: parts in 256 KiB chunks at the least)
    for s0, s1 in itertools.product(range(7), range(7)):
        for seen in (0, 128 * KIB):
            g = check(rp, (300000, 300000 + (40 << 20), 4096, seen, M.CMIN, 1 << 23, NBIG, BIG, BIG,
                           (300000 + (3 << 20) + 5, 300000 + (17 << 20)), (s0, s1)), (s0, s1, seen))
            assert g.nparts == 3 and g.parts[2].C == 4 << 20
            lo = max(M.CMIN, 2 * M.window(4096, seen, 4 * M.HMAX))
            assert g.parts[0].C == max((4 << 20) >> s0, M.pow2_from(lo, M.CMIN, 4 << 20))
            assert g.parts[1].C == max((4 << 20) >> s1, M.pow2_from(lo, M.CMIN, 4 << 20))
    # the layout's cmin above the option's cmax; cmax below RW_CMIN
    check(rp, (1000, 1 << 30, 64, 0, M.CMIN << 3, 1 << 17, NBIG, BIG, BIG, (0, 0), (0, 0)), "cmin > cmax")
    g = check(rp, (1000, 1 << 24, 4096, 0, M.CMIN, 1 << 10, NBIG, BIG, BIG, (0, 0), (0, 0)), "tiny cmax")
    assert g.parts[0].C == M.CMIN


def test_caps_force_the_chunk_to_double(rp):
    P1, length = 262200, 262200 + 64 * 65536
    # 64 chunks of 64 KiB want 64 chunks, 64 * 4 * 64 staging and 64 * 64 candidate entries at the least
    for ncap, ccap, scap, want_c in ((64, BIG, BIG, 65536), (63, BIG, BIG, 131072), (32, BIG, BIG, 131072),
                                     (31, BIG, BIG, 262144), (NBIG, 64 * 64, BIG, 65536), (NBIG, 64 * 64 - 1, BIG, 131072),
                                     (NBIG, BIG, 64 * 256, 65536), (NBIG, BIG, 64 * 256 - 1, 131072), (3, BIG, BIG, 2 << 20),
                                     (NBIG, 3 * 64, 3 * 256, 2 << 20)):
        g = check(rp, (P1, length, 60, 0, M.CMIN, 1 << 22, ncap, ccap, scap, (0, 0), (0, 0)), (ncap, ccap, scap))
        assert g.parts[0].C == want_c, (ncap, ccap, scap, g)
    # lists shrink to the caps before the chunk grows: staging 1024 -> 64, candidates 256 -> 64
    for scap in (64 * 4 * 1024, 64 * 4 * 1024 - 1, 64 * 4 * 512, 64 * 4 * 100, 64 * 4 * 64):
        g = check(rp, (P1, length, 60, 8000, M.CMIN, 1 << 22, NBIG, BIG, scap, (0, 0), (0, 0)), scap)
        assert g.parts[0].C == 65536 and g.parts[0].stgn == max(64, 1 << ((scap // 256).bit_length() - 1) if scap // 256 < 1024 else 1024)
    for ccap in (64 * 384, 64 * 384 - 1, 64 * 192, 64 * 191, 64 * 64):
        g = check(rp, (P1, length, 60, 8000, M.CMIN, 1 << 22, NBIG, ccap, BIG, (0, 0), (0, 0)), ccap)
        assert g.parts[0].H == 12288 and g.parts[0].capc == (384 if ccap >= 64 * 384 else 192 if ccap >= 64 * 192 else 96 if ccap >= 64 * 96 else 64)
    # with parts: the caps count every part's chunks
    for ncap in (3, 10, 21, 22, 40):
        check(rp, (P1, length, 60, 0, M.CMIN, 1 << 22, ncap, BIG, BIG, (P1 + 5 * 65536 + 1, P1 + 30 * 65536), (0, 0)), ncap)


def test_the_library_s_own_caps_and_cuts(rp):
    """the caps, cuts and cmax an eager call passes (model: layout_caps, split_bytes), over the lengths and
    option values of the directed stream tests"""
    for length in (1 << 20, 1310720, 1310721, 1572864, 17 << 20, (48 << 20) + 12345):
        for lead in (0, 1, 15):
            for split, split2, c0, c1 in ((8, 48, 3, 2), (0, 0, 3, 2), (1, 0, 0, 6), (128, 64, 6, 0), (100, 101, 0, 0),
                                          (64, 192, 2, 1), (255, 0, 3, 2), (40, 41, 1, 1)):
                cmin, ncap, ccap, scap = M.layout_caps(length)
                xs = M.split_bytes(length, lead, split, split2)
                cmax = min((1 << 22) << (1 if xs[0] else 0), M.CMAX)
                for mean, seen in ((60, 0), (60, 20 * KIB), (600, 70000), (20000, 65550)):
                    P1 = 262144 + 37
                    g = check(rp, (P1, length, mean, seen, cmin, cmax, ncap, ccap, scap, xs, (c0, c1) if xs[0] else (0, 0)),
                              (length, lead, split, split2, mean))
                    assert g == M.call_plan(P1, length, mean, seen, lead, split, split2, c0, c1)


def test_random_plans(rp):
    rng = np.random.default_rng(2025)
    kinds = set()
    for it in range(4000):
        P1 = int(rng.integers(0, 1 << 20))
        mean = int(rng.choice([1, 63, 64, 65, 4096, int(rng.integers(0, 100000))]))
        seen = int(rng.choice([0, 1, 4095, 4096, 128 * KIB - 4096, 128 * KIB - 4095, int(rng.integers(0, 1 << 21))]))
        cmax = 1 << int(rng.integers(16, 27))
        cmin = M.CMIN << int(rng.choice([0, 0, 0, 1, 3]))
        C0 = M.pow2_from(1024 * mean, cmin, max(cmin, cmax))
        length = P1 + int(rng.choice([1, int(rng.integers(1, 40)) * C0, int(rng.integers(1, 40)) * C0 + int(rng.integers(-1, 2)),
                                      int(rng.integers(1, 64 << 20))]))
        length = max(length, P1 + 1)
        tight = it % 4 == 0
        ncap = int(rng.integers(3, 60)) if tight else NBIG
        ccap = int(rng.integers(192, 20000)) if tight else BIG
        scap = int(rng.integers(768, 80000)) if tight else BIG
        pick = lambda: int(rng.choice([0, P1, P1 + 1, length, length + 1, P1 + C0, P1 + C0 + 1,
                                       int(rng.integers(0, length + 70000))]))
        xs = (pick(), pick())
        shifts = (int(rng.integers(0, 7)), int(rng.integers(0, 7)))
        g = check(rp, (P1, length, mean, seen, cmin, cmax, ncap, ccap, scap, xs, shifts), "random %d" % it)
        kinds.add(("parts", g.nparts))
        kinds |= {("empty", k) for k in range(g.nparts) if g.parts[k].n == 0}
        if g.parts[g.nparts - 1].C > max(cmin, cmax):
            kinds.add("doubled")
        if any(t.stgn < 256 for t in g.parts[:g.nparts]):
            kinds.add("stgn shrunk")
        if any(t.capc < t.H // 32 for t in g.parts[:g.nparts]):
            kinds.add("capc shrunk")
        want_h = M.host_plan(P1, length, mean, cmax)
        assert rp.host(P1, length, mean, cmax) == want_h, it
    assert {("parts", 1), ("parts", 2), ("parts", 3), ("empty", 0), ("empty", 1), "doubled", "stgn shrunk", "capc shrunk"} <= kinds


def test_host_linked_rule(rp):
    for mean, (c, h) in ((1, (65536, 4096)), (63, (65536, 4096)), (64, (65536, 4096)), (65, (131072, 4096)),
                         (512, (1 << 19, 4096)), (513, (1 << 20, 8192)), (4096, (1 << 22, 32768)),
                         (16384, (1 << 22, 131072)), (100000, (1 << 22, 131072))):
        got = rp.host(1000, 1000 + (9 << 20) + 1, mean, 1 << 22)
        assert got[:2] == (c, h), (mean, got)
        assert got[2] == M.ceil_div((9 << 20) + 1, c) and got[4] == h // 32
        assert got[3] == min(4096, max(256, 1 << (2 * c // mean - 1).bit_length()))
    assert rp.host(0, 20 * 65536, 60, 1 << 22)[2] == 20 and rp.host(0, 20 * 65536 + 1, 60, 1 << 22)[2] == 21


def test_a_cut_on_the_part_s_origin_leaves_it_empty(rp):
    """x == B: the part before the cut is empty and the next part starts at B, for every shift (the header
    tests `x > B`; with `>=` the round-up adds zero chunks, so both spellings give this)"""
    P1, length = 262200, 262200 + (10 << 20) + 7
    for s0, s1 in itertools.product(range(7), range(7)):
        g = check(rp, (P1, length, 4096, 0, M.CMIN, 1 << 22, NBIG, BIG, BIG, (P1, P1 + (5 << 20)), (s0, s1)), (s0, s1))
        assert g.nparts == 3 and g.parts[0].n == 0 and g.parts[1].P == P1 and g.parts[1].cbase == 0
        # ... and on the middle part's origin: x1 == the end of part 0
        e0 = P1 + (4 << 20)
        g = check(rp, (P1, length + (30 << 20), 4096, 0, M.CMIN, 1 << 22, NBIG, BIG, BIG, (P1 + (4 << 20) - 5, e0), (0, s1)), (s0, s1))
        assert g.nparts == 3 and g.parts[1].n == 0 and g.parts[1].P == e0 == g.parts[2].P
        g = check(rp, (P1, length + (30 << 20), 4096, 0, M.CMIN, 1 << 22, NBIG, BIG, BIG, (P1 + (4 << 20) - 5, e0 + 1), (0, s1)), (s0, s1))
        assert g.parts[1].n == 1
