"""GPU parity with the oracle at buffer offsets of 2^31, 2^32 and 2^33, for every device entry
point: batch decode on its four paths, reassembly (plain/Ex and Ctl, both kernel paths), the raw
stream, text validation and the host pipeline. Small inputs are placed at high offsets of one
sparse arena (tests/high_arena.py): an offset cut to 31 or 32 bits lands in a sentinel inside
the same allocation and is seen as a wrong byte. Expected values always come from the oracle on
the small input at offset 0, moved by the placement."""
import time

import numpy as np
import pytest

import dec_cases as D
import high_arena as H
import reasm_ctl_cases as RC
from oracle_lib import oracle_reassemble, oracle_segments, used_descs
from reasm_ctl_oracle import oracle_reassemble_ctl, region_image
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CATALOGUE = {cid: (fn, kw, mfs) for cid, fn, kw, mfs in D.catalogue()}
PATH_IDS = {3: "piece", 4: "segfuse", 1: "walker", -1: "auto"}
OUT_FILL = 0xEE
_cases = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def release_device_memory(dev):
    """set up first, so torn down last: the arenas and the cached cases go back to the device"""
    yield
    import gc
    _cases.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def arena(dev):
    H.need_memory(torch, pytest)
    a = H.Arena(dev)
    assert a.t.data_ptr() & 15 == 0
    yield a
    del a.t


@pytest.fixture(scope="module")
def out_arena(dev, arena):
    a = H.Arena(dev)
    yield a
    del a.t


def T64(dev, a):
    return torch.tensor(np.asarray(a, dtype=np.int64), device=dev)


# ---------------------------------------------------------------------------------- batch decode

class HighCase:
    """one wire at arena offset `high` with what the oracle says about it, computed once"""

    def __init__(self, arena, wire, so, sl, mf, high, perm=None, desc_base=None, tag=""):
        dev = arena.dev
        self.arena, self.high, self.mf, self.n, self.nseg = arena, high, mf, len(wire), len(so)
        self.tag = "%s HIGH 0x%x max_frames %d" % (tag, high, mf)
        if perm is not None:
            so, sl = [so[i] for i in perm], [sl[i] for i in perm]
        img = wire.copy()
        od, orr = oracle_segments(img, so, sl, mf, desc_base)
        self.od, self.orr = od, orr
        base = np.asarray(desc_base, np.int64) if desc_base is not None else np.arange(self.nseg, dtype=np.int64) * mf
        nslots = (int(base.max()) + mf if self.nseg else 0) + mf          # + one segment's worth of spare slots
        up = H.rebase(od, high).view(np.uint8).reshape(-1, 32)
        dimg = np.full((nslots, 32), H.SLOT_FILL, np.uint8)
        for s in range(self.nseg):
            b, k = int(base[s]), int(orr[s]["n_frames"])
            dimg[b:b + k] = up[b:b + k]
        self.pristine, self.exp = arena.framed(wire), arena.framed(img)
        self.so, self.sl = T64(dev, np.asarray(so, np.int64) + high), T64(dev, sl)
        self.db = None if desc_base is None else T64(dev, desc_base)
        self.exp_desc = arena.up(dimg.reshape(-1))
        self.exp_res = arena.up(orr.view(np.uint8).copy())
        self.desc = torch.empty_like(self.exp_desc)
        self.res = torch.empty(max(1, self.nseg) * 16, dtype=torch.uint8, device=dev)

    def run(self, what=""):
        placed = self.arena.put(self.high, self.pristine)
        self.desc.fill_(H.SLOT_FILL)
        self.res.fill_(H.SLOT_FILL)
        W.batch_decode_device(self.arena.view(self.high, self.n), self.so, self.sl, self.mf, self.desc, self.res,
                              desc_base=self.db)
        tag = self.tag + " " + what
        if not torch.equal(self.res[:self.nseg * 16], self.exp_res):
            g = self.res[:self.nseg * 16].cpu().numpy().view(W.SEGRES_DTYPE)
            s = int(np.nonzero(g != self.orr)[0][0])
            raise AssertionError("%s: result of segment %d is %s, want %s" % (tag, s, g[s], self.orr[s]))
        if not torch.equal(self.desc, self.exp_desc):
            g, e = self.desc.cpu().numpy().reshape(-1, 32), self.exp_desc.cpu().numpy().reshape(-1, 32)
            i = int(np.nonzero((g != e).any(axis=1))[0][0])
            raise AssertionError("%s: descriptor slot %d is %s, want %s (0xEE: unused)"
                                 % (tag, i, g[i].copy().view(W.DESC_DTYPE)[0], e[i].copy().view(W.DESC_DTYPE)[0]))
        self.arena.check(placed, self.exp, tag)


def cached(key, build):
    if key not in _cases:
        _cases[key] = build()
    return _cases[key]


def run_on_path(path, cases):
    W.set_option("path", path)
    try:
        for c in cases:
            c.run(PATH_IDS[path] + ", first call")
            c.run(PATH_IDS[path] + ", second call")
    finally:
        W.set_option("path", -1)


@pytest.mark.parametrize("path", list(PATH_IDS), ids=list(PATH_IDS.values()))
@pytest.mark.parametrize("bname", list(H.BOUNDARIES))
def test_byte_exact_batch_across_boundary(arena, bname, path):
    """the byte-exact batch with the boundary between every two bytes of a 14-byte header and on a
    segment start (2^31, 2^32, 2^33), and at 2^32 also on the first, the last and a mid-chunk
    payload byte, on a frame start and in a gap"""
    wire, so, sl, mf, at = H.byte_exact()
    names = list(at) if bname == "2^32" else H.header_ats(at)
    assert len(names) == (19 if bname == "2^32" else 14)
    cases = [cached(("byte_exact", bname, k), lambda k=k: HighCase(arena, wire, so, sl, mf, H.place(H.BOUNDARIES[bname], at[k]),
                                                                   tag="byte_exact %s at %s" % (bname, k))) for k in names]
    run_on_path(path, cases)


def test_byte_exact_batch_wholly_above(arena):
    wire, so, sl, mf, at = H.byte_exact()
    c = cached(("byte_exact", "above"), lambda: HighCase(arena, wire, so, sl, mf, H.ABOVE, tag="byte_exact ABOVE"))
    for path in PATH_IDS:
        run_on_path(path, [c])


ALIGNED = ["piece_edges:short", "piece_edges:long", "small_payloads", "dense_items:frames", "long_not_first",
           "segfuse_windows:edges", "run_lengths", "alphabets:ABC:sweep"]
MUST_STRADDLE = ("piece_edges:short", "piece_edges:long", "long_not_first")
HIGH_ABOVE = H.ABOVE // D.PIECE * D.PIECE


def straddled_piece(wire, so, sl, mf):
    """(a piece boundary inside the wire that a walked frame's header lies across, else one a
    payload lies across, else the middle one; what lies across it), from the oracle's descriptors"""
    od, orr = oracle_segments(wire.copy(), so, sl, mf)
    d = np.concatenate([od[s * mf:s * mf + int(orr[s]["n_frames"])] for s in range(len(so))] or [od[:0]])
    d = d[d["ret"] > 0]
    fo, hl, end = d["frame_off"].astype(np.int64), d["hdrlen"].astype(np.int64), (d["frame_off"] + d["ret"].astype(np.uint64)).astype(np.int64)
    bds = np.arange(D.PIECE, len(wire), D.PIECE)
    hdr = [int(b) for b in bds if ((fo < b) & (b < fo + hl)).any()]
    pay = [int(b) for b in bds if ((fo + hl < b) & (b < end)).any()]
    if hdr:
        return hdr[len(hdr) // 2], "header"
    if pay:
        return pay[len(pay) // 2], "payload"
    return (int(bds[len(bds) // 2]) if len(bds) else 0), None


def aligned_case(arena, cid, where, perm=False, reverse_slots=False):
    fn, kw, mfs = CATALOGUE[cid]
    wire, so, sl = fn(0, **kw)[:3]
    mf = mfs[0]
    bd, what = straddled_piece(wire, so, sl, mf)
    if cid in MUST_STRADDLE:
        assert what is not None, cid
    high = H.place_pieces(H.B32, bd) if where == "2^32" else HIGH_ABOVE
    assert high % D.PIECE == 0 and (where != "2^32" or (high < H.B32 < high + len(wire) or bd == 0))
    p, base = None, None
    if perm:
        p = np.random.default_rng(len(so)).permutation(len(so))
        assert not (np.diff(p) > 0).all()
    if reverse_slots:
        base = (np.arange(len(so), dtype=np.int64) * mf)[::-1].copy()
    c = HighCase(arena, wire, so, sl, mf, high, perm=p, desc_base=base,
                 tag="%s at %s%s%s" % (cid, where, " permuted" if perm else "", " reversed desc_base" if reverse_slots else ""))
    c.across = what
    return c


@pytest.mark.parametrize("path", list(PATH_IDS), ids=list(PATH_IDS.values()))
@pytest.mark.parametrize("where", ["2^32", "above"])
@pytest.mark.parametrize("cid", ALIGNED)
def test_directed_case_piece_aligned(arena, cid, where, path):
    """the directed catalogue placed on the piece grid, 2^32 on a piece boundary that the case
    puts a header or a payload across, and wholly above 2^32"""
    if path == 4 and CATALOGUE[cid][2][0] > 64:
        path = 3                                            # segfuse hands > 64 frames to the piece path
    c = cached((cid, where), lambda: aligned_case(arena, cid, where))
    if where == "2^32" and cid in MUST_STRADDLE:
        assert c.across in ("header", "payload")
    run_on_path(path, [c])


def test_permuted_segments_take_the_fallback_walker(arena):
    run_on_path(3, [aligned_case(arena, "piece_edges:short", "2^32", perm=True)])
    run_on_path(-1, [aligned_case(arena, "small_payloads", "above", perm=True)])


@pytest.mark.parametrize("path", list(PATH_IDS), ids=list(PATH_IDS.values()))
def test_reversed_desc_base(arena, path):
    run_on_path(path, [cached(("rev", "2^32"), lambda: aligned_case(arena, "small_payloads", "2^32", reverse_slots=True))])


# ---------------------------------------------------------------------------------- reassembly

def reasm_inputs(name):
    from test_gpu_parity import random_stream
    from test_gpu_reasm import _frame, _segments
    if name == "random":
        rng = np.random.default_rng(300)
        wire, so, sl = random_stream(rng, 300)
        return wire, so, sl, 700
    if name == "windows":                                   # test_gpu_reasm.test_reassemble_frames_across_windows
        rng = np.random.default_rng(31)
        segs = []
        for i in range(64):
            n = int(rng.integers(1, 8))
            parts = []
            for k in range(n):
                plen = int(rng.choice([20475, 20470, 20480, 40960 + 3, 65536, 70000, 100, 0, 1]))
                b0 = (0x80 if k == n - 1 else 0) | (2 if k == 0 else 0)
                parts.append(_frame(rng, plen, masked=rng.random() < 0.9, b0=b0))
            segs.append(parts)
        wire, so, sl = _segments(segs, rng)
        return wire, so, sl, 100000
    wire, limit = RC.build("limit_overflow_after_control")
    wire = np.concatenate([np.zeros(11, np.uint8), wire, np.zeros(7, np.uint8), wire[:len(wire) // 2]])
    n = (len(wire) - 18) * 2 // 3
    return wire, [11, 11 + n + 7], [n, len(wire) - 11 - n - 7], limit


def reasm_layout(way, so, sl, n, regions):
    """(wire HIGH, out base, out_off relative to the out base or None, bytes of the out window);
    2^32 falls in the middle of the longest gathered body, of its frames on the wire, or of both"""
    s = int(np.argmax([len(body) for _, body in regions]))
    half = len(regions[s][1]) // 2
    assert half > 0
    mid = int(so[s]) + half
    if way == "both_high":
        return H.place(H.B32, mid), H.place(H.B32, mid), None, n
    rel = np.zeros(len(so), np.int64)
    o = 5
    for k in reversed(range(len(so))):                      # regions in reverse order, 3 bytes apart
        rel[k] = o
        o += int(sl[k]) + 3
    if way == "wire_high":
        return H.place(H.B32, mid), 4096 + 3, rel, o
    return 4096 + 3, H.place(H.B32, int(rel[s]) + half), rel, o


@pytest.mark.parametrize("way", ["wire_high", "out_high", "both_high"])
@pytest.mark.parametrize("name", ["random", "windows", "ctl_stream"])
def test_reassembly(dev, arena, out_arena, name, way):
    """both kernel paths, through the Ex call and the Ctl call with REASM_CONTROL_DIRECT, with
    carried open / cached state and a cache limit that triggers: message descriptors (out_off
    included), bodies, state, the wire untouched, the out arena untouched outside the regions"""
    wire, so, sl, limit = reasm_inputs(name)
    mf, nseg, n = 16, len(so), len(wire)
    rng = np.random.default_rng(77)
    open0 = rng.integers(0, 2, nseg).astype(np.uint8)
    cached0 = np.where(open0 == 1, rng.integers(0, 2 * limit, nseg), 0).astype(np.uint32)
    if name == "ctl_stream":
        open0[:], cached0[:] = [0, 1], [0, limit // 2]
    wh, oh, rel, out_n = reasm_layout(way, so, sl, n, oracle_reassemble(wire, so, sl, mf, open0, None, limit, cached0)[3])
    local = None if rel is None else [int(x) for x in rel]
    assert max(wh + n, oh + out_n) >= H.B32
    so_t, sl_t = T64(dev, np.asarray(so, np.int64) + wh), T64(dev, sl)
    oo_t = None if rel is None else T64(dev, rel + oh)
    wire_t = arena.framed(wire)
    blank = out_arena.framed(np.full(out_n, OUT_FILL, np.uint8))
    for flags, oracle in ((0, oracle_reassemble), (W.REASM_CONTROL_DIRECT, oracle_reassemble_ctl)):
        od, orr, oms, oreg, oop, oca = oracle(wire, so, sl, mf, open0, local, limit, cached0)
        assert (orr["status"] == W.SEG_ERR_CACHE_OVERFLOW).any(), "the limit never triggered: the case tests nothing"
        img = np.full(out_n, OUT_FILL, np.uint8)
        for s in range(nseg):
            ob = int(so[s]) if local is None else local[s]
            if flags:
                img[ob:ob + int(sl[s])] = region_image(oreg[s], sl[s], OUT_FILL)
            else:
                img[ob:ob + len(oreg[s][1])] = oreg[s][1]
        assert (img != OUT_FILL).any()
        emsg = np.zeros(nseg * mf, W.MSG_DTYPE)
        for s in range(nseg):
            for i, m in enumerate(oms[s]):
                emsg[s * mf + i] = (m[0] + oh,) + tuple(m[1:])
        if way != "wire_high":
            assert (emsg["out_off"] + emsg["len"] > H.B32).any() and (emsg["out_off"] < H.B32).any()
        for rpath in (1, 2):
            tag = "%s %s flags %d reasm_path %d" % (name, way, flags, rpath)
            W.set_option("reasm_path", rpath)
            try:
                placed_w = arena.put(wh, wire_t)
                placed_o = out_arena.put(oh, blank)
                desc = torch.full((nseg * mf * 32,), OUT_FILL, dtype=torch.uint8, device=dev)
                msg = torch.full((nseg * mf * 32,), OUT_FILL, dtype=torch.uint8, device=dev)
                res = torch.zeros(nseg * 16, dtype=torch.uint8, device=dev)
                nmsg = torch.zeros(nseg, dtype=torch.int32, device=dev)
                op = torch.tensor(open0, device=dev)
                ca = torch.tensor(cached0.view(np.int32), device=dev)
                W.batch_reassemble_device(arena.view(wh, n), so_t, sl_t, mf, desc, res, out_arena.t, msg, nmsg, out_off=oo_t,
                                          open_state=op, readcache_max=limit, cached=ca, flags=flags)
                torch.cuda.synchronize()
            finally:
                W.set_option("reasm_path", 0)
            gr = res.cpu().numpy().view(W.SEGRES_DTYPE)
            gd, gm, gn = desc.cpu().numpy().view(W.DESC_DTYPE), msg.cpu().numpy().view(W.MSG_DTYPE), nmsg.cpu().numpy()
            assert np.array_equal(gr, orr), tag
            assert np.array_equal(used_descs(gd, gr, mf), H.rebase(used_descs(od, orr, mf), wh)), tag
            assert [int(x) for x in gn] == [len(m) for m in oms], tag
            for s in range(nseg):
                k = len(oms[s])
                assert np.array_equal(gm[s * mf:s * mf + k], emsg[s * mf:s * mf + k]), (tag, s, gm[s * mf:s * mf + k],
                                                                                     emsg[s * mf:s * mf + k])
            assert np.array_equal(op.cpu().numpy(), oop), tag
            assert np.array_equal(ca.cpu().numpy().view(np.uint32), oca), tag
            arena.check(placed_w, wire_t, tag + ": the wire")
            out_arena.check(placed_o, img, tag + ": the out arena")


# ---------------------------------------------------------------------------------- raw stream

SLICE = 256 << 20


def test_raw_stream_past_4gib(dev, arena, out_arena):
    """one raw stream of 2^32 + ~2 MiB: three masked frames of under 2^31 wire bytes each up to
    about 1 MiB short of 2^32 (payloads random, written on the device in 256 MiB slices), then the
    cfg3 length mix, small frames across 2^32 and the mix again above it. The big frames'
    descriptors are analytic, the tail's the oracle's moved by the tail's offset; the big payloads
    are compared on the device slice by slice as wire ^ key. Eager with the chunk-parallel walk,
    with the serial walk, with max_frames stopping just past 2^32, and truncated 999 bytes short."""
    from test_gpu_stream import long_stream, mix3
    t0 = time.time()
    rng = np.random.default_rng(4096)
    part1 = long_stream(rng, (1 << 20) - (70 << 10), mix3)
    tail = np.concatenate([part1, long_stream(rng, 8000, lambda g: g.integers(0, 301)), long_stream(rng, 2 << 20, mix3)])
    t = H.B32 - len(part1) - 4000                                         # where the tail starts
    total = t + len(tail)
    w3 = 300007
    w1 = H.B31 - 5003
    w2 = t - w1 - w3
    assert 14 < w2 < H.B31 and total + 64 <= H.ARENA_BYTES
    keys = [bytes([0x11, 0x22, 0x33, 0x44]), bytes([0xA1, 0x02, 0xF3, 0x74]), bytes([0x5A, 0xC3, 0x0F, 0x96])]
    starts = [0, w1, w1 + w3]
    lens = [w1, w3, w2]
    a, b = arena.t, out_arena.t                                          # b keeps the wire as it was
    g = torch.Generator(device=dev)
    g.manual_seed(65)
    for x in range(0, t, SLICE):
        y = min(x + SLICE, t)
        b[x:y] = torch.randint(0, 256, (y - x,), dtype=torch.uint8, device=dev, generator=g)
    for st, ln, key in zip(starts, lens, keys):
        hdr = bytes([0x82, 0x80 | 127]) + (ln - 14).to_bytes(8, "big") + key
        b[st:st + 14] = arena.up(np.frombuffer(hdr, np.uint8).copy())
    b[t:total] = arena.up(tail)
    b[total:total + 64] = 0
    ot = tail.copy()
    tail_mf = 1 << 12
    od, orr = oracle_segments(ot, [0], [len(tail)], tail_mf)
    nt = int(orr[0]["n_frames"])
    assert int(orr[0]["status"]) == W.SEG_OK and int(orr[0]["consumed"]) == len(tail) and nt < tail_mf - 3
    fo = od["frame_off"][:nt].astype(np.int64) + t
    assert (fo < H.B32).any() and ((fo < H.B32) & (fo + od["ret"][:nt] > H.B32)).any() and (fo > H.B32).sum() > 30
    big = np.zeros(3, W.DESC_DTYPE)
    for i, (st, ln) in enumerate(zip(starts, lens)):
        big[i] = (st, st + 14, ln - 14, ln, 1, 2, 1, 14)
    full = np.concatenate([big, H.rebase(od[:nt], t)])
    first_above = 3 + int(np.nonzero(fo >= H.B32)[0][0])

    def variant(length, mf, rw, what):
        a[:total + 64] = b[:total + 64]
        desc = torch.full((mf * 32,), 0xEE, dtype=torch.uint8, device=dev)
        res = torch.zeros(16, dtype=torch.uint8, device=dev)
        W.set_option("stream_rw", rw)
        try:
            W.stream_decode_device(a[:length + 64], length, mf, desc, res)
            torch.cuda.synchronize()
        finally:
            W.set_option("stream_rw", 1)
        gr = res.cpu().numpy().view(W.SEGRES_DTYPE)[0]
        # the expected walk: the oracle over the tail's share of [0, length) with the frames left
        et = tail.copy()
        ed, er = oracle_segments(et, [0], [length - t], mf - 3)
        en = int(er[0]["n_frames"])
        want = (t + int(er[0]["consumed"]), 3 + en, int(er[0]["status"]))
        assert (int(gr["consumed"]), int(gr["n_frames"]), int(gr["status"])) == want, what
        gd = desc.cpu().numpy().view(W.DESC_DTYPE)
        exp = np.concatenate([big, H.rebase(ed[:en], t)])
        bad = np.nonzero(gd[:3 + en] != exp)[0]
        assert len(bad) == 0, (what, int(bad[0]), gd[bad[0]], exp[bad[0]])
        assert (desc[(3 + en) * 32:] == 0xEE).all(), what + ": descriptor slots past n_frames written"
        assert torch.equal(a[t:total + 64], arena.up(np.concatenate([et, np.zeros(64, np.uint8)]))), what + ": the tail"
        for st, ln, key in zip(starts, lens, keys):
            assert torch.equal(a[st:st + 14], b[st:st + 14]), what + ": a big frame's header"
            p0 = st + 14
            tile = arena.up(np.frombuffer(key, np.uint8).copy()).repeat(SLICE // 4)
            for x in range(p0, st + ln, SLICE):                              # SLICE % 4 == 0: the key phase restarts
                y = min(x + SLICE, st + ln)
                assert bool((a[x:y] == (b[x:y] ^ tile[:y - x])).all()), "%s: big payload differs in [%d, %d)" % (what, x, y)
            del tile
        return want

    times = {}
    for what, args in (("chunk-parallel walk", (total, 1 << 12, 1)), ("serial walk", (total, 1 << 12, 0)),
                       ("max_frames just past 2^32", (total, first_above + 2, 1)),
                       ("999 bytes short", (total - 999, 1 << 12, 1))):
        t1 = time.time()
        want = variant(*args, what)
        times[what] = time.time() - t1
        if what.startswith("max_frames"):
            assert want[2] == W.SEG_MAX_FRAMES and want[0] > H.B32
        elif what.startswith("999"):
            assert want[0] < total - 999
        else:
            assert want == (total, 3 + nt, W.SEG_OK)
    print("raw stream past 4 GiB: set-up %.2f s, %s" % (time.time() - t0 - sum(times.values()),
                                                        ", ".join("%s %.2f s" % kv for kv in times.items())))


# ---------------------------------------------------------------------------------- text

@pytest.mark.parametrize("where", ["straddle", "above"])
def test_text_validation_high_out_off(dev, out_arena, where):
    """test_gpu_text's lengths-and-phases, sequences-across-every-edge and carry-between-batches
    cases with every out_off at or around 2^32: 2^32 inside a body, and the layout from ABOVE on"""
    import test_gpu_text as TT
    from util_amd import _lib
    _lib.load_text_lib()
    base = H.B32 - 40000 if where == "straddle" else H.ABOVE
    assert base % 16 == (0 if where == "straddle" else 5)
    TT.lengths_and_phases(dev, arena=out_arena, base=base)
    TT.sequences_across_every_edge(dev, arena=out_arena, base=base)
    TT.carry_between_batches(dev, arena=out_arena, base=H.B32 - 1000 if where == "straddle" else H.ABOVE)


# ---------------------------------------------------------------------------------- host path

@pytest.fixture(scope="module")
def host_buf():
    b = np.empty(2**32 + (16 << 20), np.uint8)             # only the pages that are used get touched
    yield b
    del b


@pytest.mark.parametrize("where", ["straddle", "above"])
def test_host_path_high(dev, host_buf, where):
    """websocketframeBatchDecodeHost (1 MiB groups), HostMulti on [0, 0, 0] and permuted segments
    on a host buffer of 2^32 + 16 MiB with 2^32 inside a segment, and wholly above it"""
    from test_gpu_parity import random_stream
    rng = np.random.default_rng(2001)
    wire, so, sl = random_stream(rng, 2001, max_frame=30000)
    n, mf = len(wire), 16
    assert H.ABOVE + n + 64 <= len(host_buf)                # 11.5 MB of wire: 8 MiB past 2^32 would not hold it
    s_mid = next(s for s in range(len(so) // 2, len(so)) if sl[s] > 2000)
    high = H.place(H.B32, so[s_mid] + sl[s_mid] // 2) if where == "straddle" else H.ABOVE
    so_h = np.asarray(so, np.uint64) + np.uint64(high)
    sl_h = np.asarray(sl, np.uint64)
    perm = rng.permutation(len(so))
    W.set_option("host_chunk_mb", 1)
    try:
        for what, call, p in (("host", lambda b, o, l: W.batch_decode_host(b, o, l, mf), None),
                              ("multi", lambda b, o, l: W.batch_decode_host_multi(b, o, l, mf, [0, 0, 0]), None),
                              ("permuted", lambda b, o, l: W.batch_decode_host(b, o, l, mf), perm),
                              ("multi permuted", lambda b, o, l: W.batch_decode_host_multi(b, o, l, mf, [0, 0, 0]), perm)):
            o_, l_ = (so_h, sl_h) if p is None else (so_h[p], sl_h[p])
            lo_, ll_ = (so, sl) if p is None else ([so[i] for i in p], [sl[i] for i in p])
            host_buf[high - 64:high + n + 64] = H.framed(wire)
            gd, gr = call(host_buf, o_, l_)
            ob = wire.copy()                               # gaps included: bytes between segments untouched
            od, orr = oracle_segments(ob, lo_, ll_, mf)
            assert np.array_equal(gr, orr), what
            assert np.array_equal(used_descs(gd, gr, mf), H.rebase(used_descs(od, orr, mf), high)), what
            got = host_buf[high - 64:high + n + 64]
            bad = np.nonzero(got != H.framed(ob))[0]
            assert len(bad) == 0, (what, "first differing byte at wire offset", int(bad[0]) - 64)
            for k in range(len(so)):
                assert not gd[k * mf + int(gr[k]["n_frames"]):(k + 1) * mf].view(np.uint8).any(), what
    finally:
        W.set_option("host_chunk_mb", 64)
