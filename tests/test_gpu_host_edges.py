"""GPU parity of the host-memory decode (websocketframeBatchDecodeHost / ...HostMulti) on directed
batches (tests/host_cases.py): every branch of the host plan (groups closed by bytes and by the
descriptor cap, empty segments in every position, gaps, 1-7 groups over the three slots, unordered
segments), the geometric families of dec_cases.py laid at host offsets so the group's device buffer
(slot - lo) sees them at their designed phases, slot growth across calls, one call whose groups take
different decode paths, every multi-device cut cell, and the clean error returns. Every call is
compared in full with the oracle: the whole host image (bytes before, between and after the
segments are 0xA5 and must come back untouched), results, used descriptors, zeros in the unused
slots, and the "host_groups" counter against the model's group count; twice in a row (slot state
and hints carry over), on "path" -1, 3, 4 and 1."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import host_cases as H
from oracle_lib import oracle_segments
from util_amd import _lib
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
PLAN = {L.name: L for L in H.plan_layouts() if L.gpu and L.name != "outside"}    # "outside": test_error_returns
CUTS = {L.name: L for L in H.cut_layouts()}
_want = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def one_mib_groups(dev):
    W.set_option("host_chunk_mb", 1)
    try:
        yield
    finally:
        W.set_option("host_chunk_mb", 64)
        W.set_option("path", -1)


@pytest.fixture(scope="module", autouse=True)
def drop_references(dev):
    yield
    _want.clear()
    H._filled.clear()


def paths_for(mf):
    return [p for p in (-1, 3, 4, 1) if not (p == 4 and mf > 64)]


def want(key, image, so, sl, mf):
    """(oracle image, results, descriptor bytes with zeros in the unused slots), computed once per key"""
    if key not in _want:
        img = image.copy()
        od, orr = oracle_segments(img, so, sl, mf)
        nseg = len(so)
        dimg = np.zeros((max(1, nseg * mf), 32), np.uint8)
        if nseg:
            used = (np.arange(mf, dtype=np.uint32)[None, :] < orr["n_frames"][:, None]).reshape(-1)
            dimg[:nseg * mf][used] = od[:nseg * mf].view(np.uint8).reshape(-1, 32)[used]
        _want[key] = (img, orr.copy(), dimg)
    return _want[key]


def host_buffer(image, pinned):
    if not pinned:
        return image.copy()
    t = torch.empty(len(image), dtype=torch.uint8, pin_memory=True)
    hb = t.numpy()
    hb[:] = image
    return hb


def check_call(key, image, so, sl, mf, devices=None, chunk=H.MIB, pinned=False, paths=None, repeat=2):
    """one host call compared in full with the oracle, on every path, `repeat` times in a row"""
    img, orr, dimg = want(key, image, so, sl, mf)
    groups = H.model_groups(list(so), list(sl), mf, len(image), chunk, None if devices is None else len(devices))
    so_a, sl_a = np.asarray(so, np.uint64), np.asarray(sl, np.uint64)
    for path in paths or paths_for(mf):
        W.set_option("path", path)
        for rep in range(repeat):
            tag = "%s path %d call %d%s" % (key, path, rep + 1, "" if devices is None else " devices %s" % (devices,))
            hb = host_buffer(image, pinned)
            g0 = W.get_stat("host_groups")
            if devices is None:
                gd, gr = W.batch_decode_host(hb, so_a, sl_a, mf)
            else:
                gd, gr = W.batch_decode_host_multi(hb, so_a, sl_a, mf, devices)
            assert W.get_stat("host_groups") - g0 == groups, tag
            if not np.array_equal(gr, orr):
                s = int(np.nonzero(gr != orr)[0][0])
                raise AssertionError("%s: result of segment %d is %s, want %s" % (tag, s, gr[s], orr[s]))
            g8 = gd.view(np.uint8).reshape(-1, 32)
            if not np.array_equal(g8, dimg):
                i = int(np.nonzero((g8 != dimg).any(axis=1))[0][0])
                raise AssertionError("%s: descriptor slot %d (segment %d, frame %d) is %s, want %s (zeros: unused)"
                                     % (tag, i, i // mf, i % mf, gd[i], dimg[i].copy().view(W.DESC_DTYPE)[0]))
            if not np.array_equal(hb, img):
                bad = np.nonzero(hb != img)[0]
                p = int(bad[0])
                inside = any(o <= p < o + n for o, n in zip(so, sl))
                raise AssertionError("%s: %d host bytes differ, first at offset %d (%s): got 0x%02x, want 0x%02x"
                                     % (tag, len(bad), p, "inside a segment" if inside else "outside every segment",
                                        int(hb[p]), int(img[p])))
    W.set_option("path", -1)


# ---------------------------------------------------------------------------------- the plan's branches

@pytest.mark.parametrize("name", list(PLAN))
def test_directed_plan_layout(dev, name):
    L = PLAN[name]
    check_call(name, H.filled(L), L.so, L.sl, L.max_frames)


def test_pinned_host_memory(dev):
    """three groups over three slots, once more from pinned memory (asynchronous DMA, not staging copies)"""
    L = PLAN["groups_3"]
    check_call(L.name, H.filled(L), L.so, L.sl, L.max_frames, pinned=True)
    L = PLAN["zero_positions"]
    check_call(L.name, H.filled(L), L.so, L.sl, L.max_frames, pinned=True, paths=[-1])


# ---------------------------------------------------------------------------------- lo geometry

@pytest.mark.parametrize("variant", ["open", "spacer"])
@pytest.mark.parametrize("cid", H.GEOM)
def test_lo_geometry(dev, cid, variant):
    """the case in one group that starts at lo (host_cases part 4 derives lead0), lo at each phase of
    {0, 1, 8, 15}; a case longer than 1 MiB needs the group size that holds it, and is then run at
    1 MiB as well (several groups, each at a phase of its own: parity only)"""
    if variant == "open" and cid in H.GEOM_NO_OPEN:
        assert H.placed(cid, H.LO_BASES[0], variant) is None
        return
    for lo in H.LO_BASES:
        assert lo % 16 in (0, 1, 8, 15) and lo % 16384
        image, so, sl, mf, lead0 = H.placed(cid, lo, variant)
        assert min(so) == so[0] == lo
        mb = max(1, -(-(so[-1] + sl[-1] - lo) // H.MIB))
        assert H.model_groups(so, sl, mf, len(image), mb * H.MIB) == 1
        key = "%s %s lo %d" % (cid, variant, lo)
        W.set_option("host_chunk_mb", mb)
        check_call(key, image, so, sl, mf, chunk=mb * H.MIB)
        if mb > 1:
            W.set_option("host_chunk_mb", 1)
            check_call(key, image, so, sl, mf, paths=[-1], repeat=1)
        del _want[key]


# ---------------------------------------------------------------------------------- slot state across calls

def test_slot_growth_across_calls(dev):
    """small, then larger in span, segment count and max_frames (4 -> 64), then small again: the slots
    grow once and the small call runs in oversized slots"""
    small, big = H.growth_layouts()
    ps = H.plan(small.so, small.sl, small.max_frames, small.buflen, H.MIB)[1]
    pb = H.plan(big.so, big.sl, big.max_frames, big.buflen, H.MIB)[1]
    assert len(ps) == 3 and len(pb) >= 3 and big.max_frames > small.max_frames
    assert min(hi - lo for _, _, lo, hi in pb) > max(hi - lo for _, _, lo, hi in ps)
    assert min(s1 - s0 for s0, s1, _, _ in pb) > max(s1 - s0 for s0, s1, _, _ in ps)
    for path in (-1, 3, 4, 1):
        for L in (small, big, small):
            check_call(L.name, H.filled(L), L.so, L.sl, L.max_frames, paths=[path], repeat=1)


def segfuse_fits_rule():
    """ws_segfuse_fits restated, its constants read from ws_segfuse.hip"""
    with open(os.path.join(os.path.dirname(HERE), "util_amd", "csrc", "ws_segfuse.hip")) as f:
        src = f.read()
    tb = int(re.search(r"#define SF_TB (\d+)", src).group(1))
    m = re.search(r"max_frames <= SF_TB && nseg >= (\d+) && span <= \(u64\)nseg \* \(\((\d+)u << 10\) - (\d+)\)", src)
    nmin, kib, less = (int(x) for x in m.groups())
    return lambda span, nseg, mf: mf <= tb and nseg >= nmin and span <= nseg * ((kib << 10) - less)


@pytest.mark.parametrize("layout", [L.name for L in H.mixed_layouts()])
@pytest.mark.parametrize("state", ["unprimed", "primed"])
def test_mixed_paths_in_one_call(dev, state, layout):
    """one call under "path" -1 whose groups take different decode paths: the largest span and the
    largest segment count over the groups fit the segment-fused path (no workspace), one group does
    not (the piece path, which needs one). In a fresh process, as its first host call and after a
    call that left a small piece workspace in all three slots: the slots' workspace must follow each
    group's path. (Sized from the maxima, the primed call returned "workspace too small" with the
    first group already written back.)"""
    fits = segfuse_fits_rule()
    L = {x.name: x for x in H.mixed_layouts()}[layout]
    groups = H.plan(L.so, L.sl, L.max_frames, L.buflen, H.MIB)[1]
    assert fits(max(hi - lo for _, _, lo, hi in groups), max(s1 - s0 for s0, s1, _, _ in groups), L.max_frames)
    assert sum(1 for s0, s1, lo, hi in groups if not fits(hi - lo, s1 - s0, L.max_frames)) >= 1
    assert sum(1 for s0, s1, lo, hi in groups if fits(hi - lo, s1 - s0, L.max_frames)) >= 1
    P = H.prime_layout()
    pg = H.plan(P.so, P.sl, P.max_frames, P.buflen, H.MIB)[1]
    assert len(pg) == 3 and P.max_frames == 4 and all(s1 - s0 == 10 for s0, s1, _, _ in pg)
    r = subprocess.run([sys.executable, os.path.join(HERE, "host_mixed_child.py"), state, layout], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    ok = {"rc": 0, "image": True, "res": True, "desc": True}
    if state == "primed":
        assert out["prime"] == ok, out
    assert out["host"] == ok and out["multi"] == ok, out


# ---------------------------------------------------------------------------------- several devices

@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0], [0] * 7], ids=["2", "3", "7"])
def test_multi_device_cut_cells(dev, devices):
    for L in CUTS.values():
        check_call(L.name, H.filled(L), L.so, L.sl, L.max_frames, devices=devices)
        if 1 in L.ndevs and len(devices) == 2:
            check_call(L.name, H.filled(L), L.so, L.sl, L.max_frames, devices=[0], paths=[-1])
    for name in ("groups_3", "zero_positions"):                # ranges that are cut into groups in turn
        L = PLAN[name]
        check_call(name, H.filled(L), L.so, L.sl, L.max_frames, devices=devices, paths=[-1])


# ---------------------------------------------------------------------------------- error returns

def raw_call(entry, hb, so, sl, mf, desc, res, device):
    lib = _lib.load_lib()
    so_a, sl_a = np.ascontiguousarray(so, dtype=np.uint64), np.ascontiguousarray(sl, dtype=np.uint64)
    if entry == "websocketframeBatchDecodeHost":
        rc = lib.websocketframeBatchDecodeHost(hb.ctypes.data, hb.nbytes, so_a.ctypes.data, sl_a.ctypes.data, len(so), mf,
                                               desc.ctypes.data, res.ctypes.data, device)
    else:
        devs = np.ascontiguousarray(device, dtype=np.int32)
        rc = lib.websocketframeBatchDecodeHostMulti(hb.ctypes.data, hb.nbytes, so_a.ctypes.data, sl_a.ctypes.data, len(so),
                                                    mf, desc.ctypes.data, res.ctypes.data, devs.ctypes.data, len(devs))
    return rc, lib.websocketframeGpuLastError().decode(errors="replace")


def test_error_returns(dev):
    """a nonzero return, a message that names the entry point, h_buf / h_desc / h_res untouched, and
    the next valid call bit-exact"""
    good = PLAN["groups_2"]
    bad = {L.name: L for L in H.plan_layouts()}["outside"]
    one, multi = "websocketframeBatchDecodeHost", "websocketframeBatchDecodeHostMulti"
    cases = [("segment outside the buffer", one, bad, bad.max_frames, 0, "segment outside buffer"),
             ("segment outside the buffer", multi, bad, bad.max_frames, [0, 0], "segment outside buffer"),
             ("max_frames 0", one, good, 0, 0, "invalid argument"),
             ("max_frames 0", multi, good, 0, [0, 0], "invalid argument"),
             ("device -1", one, good, good.max_frames, -1, "device"),
             ("device 64", one, good, good.max_frames, 64, "device"),
             ("devices [0, 64]", multi, good, good.max_frames, [0, 64], "device 64"),
             ("devices [-1, 0]", multi, good, good.max_frames, [-1, 0], "device -1")]
    for what, entry, L, mf, device, word in cases:
        image = H.filled(L)
        hb = image.copy()
        desc = np.full(len(L.so) * max(mf, 1) * 32, 0xEE, np.uint8)
        res = np.full(len(L.so) * 16, 0xEE, np.uint8)
        rc, msg = raw_call(entry, hb, L.so, L.sl, mf, desc, res, device)
        assert rc != 0, what
        assert entry in msg and word in msg, (what, msg)
        assert np.array_equal(hb, image) and (desc == 0xEE).all() and (res == 0xEE).all(), what
        check_call(good.name, H.filled(good), good.so, good.sl, good.max_frames, paths=[-1], repeat=1)
        check_call(good.name, H.filled(good), good.so, good.sl, good.max_frames, devices=[0, 0], paths=[-1], repeat=1)
