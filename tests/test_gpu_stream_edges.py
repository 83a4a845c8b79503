"""GPU parity of websocketframeStreamDecodeDevice on the directed cases of tests/stream_cases.py: chunk
starts, windows, long frames, the stream's end, max_frames, bad headers and the split options on a
1.25 MiB stream whose every chunk edge the model of tests/rwplan_model.py computes. Each case: result,
descriptors and every byte against the oracle, as test_gpu_stream.run does — with valid masked frames
before the buffer and after its end (a read past either end that reached a verdict shows) and a guard
after the descriptors — and the plan the call chose, read back through the "stream_plan_*" stats, equal
to the model's, with the case's cells true under it. A case whose geometry did not come out as claimed
fails."""
import numpy as np
import pytest

import rwplan_model as M
import stream_cases as S
from oracle_lib import oracle_segments
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAD = np.frombuffer(bytes([0x82, 0x80, 0x11, 0x22, 0x33, 0x44]) * 16, dtype=np.uint8)   # zero-length masked frames
GUARD = 256


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def stream_opts():
    """restores the raw stream's options after a test that changes them"""
    yield
    for k, v in S.DEFAULT_OPTS.items():
        W.set_option(k, v)
    W.set_option("stream_rw", 1)
    W.set_option("stream_plink", 1)


class Bufs:
    """one device buffer, descriptor array and result shared by a group's cases"""

    def __init__(self, dev, nbytes=S.BASE_BYTES, max_frames=S.BIG_MF, stream=None):
        self.dev = dev
        self.stream = stream                                   # a torch stream of its own (default: the current one)
        self.max_frames = max_frames
        self.d = torch.zeros(16 + nbytes + 64, dtype=torch.uint8, device=dev)
        self.desc = torch.zeros(max_frames * 32 + GUARD, dtype=torch.uint8, device=dev)
        self.res = torch.zeros(16, dtype=torch.uint8, device=dev)
        assert self.d.data_ptr() % 16 == 0

    def run(self, wire, max_frames, shift=0):
        """decode and compare with the oracle; returns the result"""
        n = len(wire)
        host = np.empty(shift + n + 64, dtype=np.uint8)
        host[:shift] = PAD[len(PAD) - shift:] if shift else []
        host[shift:shift + n] = wire
        host[shift + n:] = PAD[:64]
        self.d[:len(host)].copy_(torch.from_numpy(host))
        self.desc.fill_(0xEE)
        self.res.zero_()
        if self.stream is None:
            W.stream_decode_device(self.d[shift:], n, max_frames, self.desc, self.res)
        else:
            torch.cuda.synchronize()
            with torch.cuda.stream(self.stream):
                W.stream_decode_device(self.d[shift:], n, max_frames, self.desc, self.res, stream=self.stream)
        torch.cuda.synchronize()
        gr = self.res.cpu().numpy().view(W.SEGRES_DTYPE)[0]
        ob = wire.copy()
        od, orr = oracle_segments(ob, [0], [n], max_frames)
        assert tuple(gr) == tuple(orr[0]), (tuple(gr), tuple(orr[0]))
        nf = int(gr["n_frames"])
        dh = self.desc.cpu().numpy()
        assert np.array_equal(dh[:nf * 32].view(W.DESC_DTYPE), od[:nf])
        assert (dh[max_frames * 32:max_frames * 32 + GUARD] == 0xEE).all(), "descriptors written past max_frames"
        got = self.d[:len(host)].cpu().numpy()
        assert np.array_equal(got[:shift], host[:shift]) and np.array_equal(got[shift + n:], host[shift + n:]), "bytes outside the stream changed"
        if not np.array_equal(got[shift:shift + n], ob):
            bad = np.nonzero(got[shift:shift + n] != ob)[0]
            raise AssertionError("%d bytes differ, first at %d" % (len(bad), bad[0]))
        return gr


def read_plan():
    """the last chunk-planned call's plan as a model Geom (+ path, active, nf, per-part link facts)"""
    st = lambda name: W.get_stat("stream_plan_" + name)
    parts, cb, sb, db = [], 0, 0, 0
    link = []
    for k in range(M.NP):
        P, Cc, H, n, capc, stgn = (st("%s%d" % (f, k)) for f in ("P", "C", "H", "n", "capc", "stgn"))
        parts.append(M.Part(P, Cc, H, n, cb, capc, stgn, sb, db))
        cb, sb, db = cb + n, sb + n * M.OWNERS * stgn, db + n * capc
        link.append(dict(nrows=st("nrows%d" % k), linked=st("linked%d" % k), serial=st("lk_serial%d" % k),
                         walks=st("lk_walks%d" % k), in_state=st("in_state%d" % k), in_ent=st("in_ent%d" % k),
                         in_nf=st("in_nf%d" % k)))
    return dict(geom=M.Geom(parts, st("nparts"), st("nchunks")), path=st("path"), active=st("active"), nf=st("nf"), link=link)


def condition(bufs):
    """the base stream on the same torch stream, twice if need be: the walk hint is set (lengths keep
    changing) and the next call's `seen` is the base's longest frame after the sample"""
    wire, fo, fl = S.base_stream()
    n0 = W.get_stat("stream_skips")
    bufs.run(wire, S.BIG_MF)
    if W.get_stat("stream_skips") != n0 + 1:
        n0 = W.get_stat("stream_skips")
        bufs.run(wire, S.BIG_MF)
        assert W.get_stat("stream_skips") == n0 + 1, "the base stream did not set the walk hint"
    _, P1, _ = S.base_chunks()
    return int(fl[np.searchsorted(fo, P1):].max())


def check_plan(case, shift, seen, opts, what):
    """the plan read back equals the model's for this case, and the case's cells hold under it"""
    fo, fl, res = S.frame_offsets(case.wire)
    if case.max_frames != S.BIG_MF:
        res = S.frame_offsets(case.wire, case.max_frames)[2]
    want = S.geometry(case.wire, seen=seen, lead=shift, opts=opts, fo=fo, fl=fl)
    plan = read_plan()
    assert plan["path"] == 1, (what, case.name)
    nsample = int(np.searchsorted(fo, M.SAMPLE))
    if want is None or case.max_frames < nsample:                # the walk ended in the sample or never reached chunks
        # (max_frames == the sample's count: the sample walk stops at its end first, the plan is made)
        assert plan["active"] == 0, (what, case.name, plan)
        return plan
    g, P1, nf = want
    assert plan["active"] == 1 and plan["nf"] == nf, (what, case.name, plan["nf"], nf)
    assert plan["geom"] == g, (what, case.name, plan["geom"], g)
    for cell in case.cells:
        S.check_cell(cell, case.wire, case.max_frames, plan["geom"], fo, fl, res, lead=shift)
    return plan


def clear_hint(bufs):
    """a uniform stream longer than 512 KiB on the same torch stream: whichever way it is decoded (the pass
    rounds confirm it, or a chunk walk's sample sees runs), the next call starts with its pass rounds"""
    uni = np.frombuffer(S.uniform(np.random.default_rng(6), 9000, 60), dtype=np.uint8).copy()
    assert len(uni) >= M.MIN_STREAM
    bufs.run(uni, S.BIG_MF)
    n0 = W.get_stat("stream_skips")
    bufs.run(uni, S.BIG_MF)
    assert W.get_stat("stream_skips") == n0, "the hint was not cleared"


def run_case(bufs, case, shift=0, cond=True, seen=0):
    """condition (unless the caller did), decode the case on the skip path, compare with the oracle, read the
    plan back and hold it against the model"""
    opts = dict(S.DEFAULT_OPTS, **(case.opts or {}))
    if cond:
        for k, v in S.DEFAULT_OPTS.items():
            W.set_option(k, v)
        seen = condition(bufs)
    for k, v in opts.items():
        W.set_option(k, v)
    n0 = W.get_stat("stream_skips")
    bufs.run(case.wire, case.max_frames, shift)
    assert W.get_stat("stream_skips") == n0 + 1, (case.name, "not the skip path")
    return check_plan(case, shift, seen, opts, "eager")


@pytest.fixture(scope="module")
def bufs(dev):
    return Bufs(dev)


def test_plan_stats_of_the_base_stream(bufs, stream_opts):
    """the plan read back is the model's; every chunk of the live part was linked from a record or walked by
    the serial linker, which then says so (windows of 8 KiB hold more than RW_S0 starts of 26-96 B frames, so
    whether the entry's record got a slot is the hardware's order); unknown names are refused"""
    plan = run_case(bufs, S.Case("base", S.base_stream()[0], S.BIG_MF, [("split", "part0_empty")], None))
    last = plan["geom"].nparts - 1
    L = plan["link"][last]
    assert L["linked"] == 1 and L["nrows"] + L["walks"] == plan["geom"].parts[last].n, L
    assert L["serial"] == 1 or L["walks"] == 0, L
    for bad in ("stream_plan_", "stream_plan_P3", "stream_plan_nope0", "stream_plan_P"):
        with pytest.raises(ValueError):
            W.get_stat(bad)


@pytest.mark.parametrize("group", ["chunk_start", "window_long", "stream_end", "counts", "endings", "splits", "handoffs",
                                   "aligned", "pools"])
def test_directed_group(bufs, stream_opts, group):
    for i, case in enumerate(S.cases(group)):
        plan = run_case(bufs, case, shift=(0, 3, 15, 8)[i % 4] if group == "chunk_start" else 0)
        g = plan["geom"]
        if group in ("splits", "aligned"):                     # every hand-off happened, at or past the part's origin
            for k in range(1, g.nparts):
                assert plan["link"][k]["in_state"] == 1 and plan["link"][k]["in_ent"] >= g.parts[k].P, (case.name, k)
        for cell in case.cells:
            if cell[0] == "max_at" and cell[1].startswith("handoff"):
                k, d, want = int(cell[1][-1]), cell[2], cell[3]
                L = plan["link"][k]
                # one frame more than in_nf: the part is entered with in_nf frames before it; one fewer: the walk
                # ended before it; exactly in_nf: either (a part whose last chunk's count meets max_frames
                # may still hand over, and the next part then ends on its first candidate) — exact both ways
                if d > 0 or (d == 0 and L["in_state"] == 1):
                    assert (L["in_state"], L["in_nf"]) == (1, want), (case.name, L)
                else:
                    assert L["in_state"] == 2, (case.name, L)
            if cell[0] == "end" and cell[2].startswith("part"):
                L = plan["link"][int(cell[2][-1])]
                assert L["in_state"] == 1 and L["in_ent"] == cell[4], (case.name, L)


@pytest.mark.parametrize("which", [0, 1])
def test_stream_end_at_every_phase(bufs, stream_opts, which):
    """the stream-end cells at the 16 phases of (base + len) mod 16: every buffer shift 0..15"""
    cs = S.cases("stream_end")
    mine = cs[:6] + cs[12:15] if which == 0 else cs[6:12] + cs[15:]
    condition(bufs)
    for case in mine:
        for shift in range(16):
            run_case(bufs, case, shift=shift, cond=False, seen=96)


def test_window_entry_past_the_window_is_walked(bufs, stream_opts):
    """the chain's first frame start one byte past the window: the window holds no entry, so the serial
    linker links the part and walks those two chunks itself"""
    by = {c.name: c for c in S.cases("window_long")}
    plan = run_case(bufs, by["entry_8192"])
    last = plan["geom"].nparts - 1
    assert plan["link"][last]["serial"] == 1 and plan["link"][last]["walks"] >= 2, plan["link"]


def representatives():
    return [S.cases("chunk_start")[0], S.cases("chunk_start")[4], S.cases("window_long")[1], S.cases("window_long")[5],
            S.cases("stream_end")[1], S.cases("counts")[4], S.cases("endings")[2], S.cases("splits")[-2],
            S.cases("handoffs")[2]]


def test_representatives_through_the_serial_linker(bufs, stream_opts):
    for case in representatives():
        W.set_option("stream_plink", 0)
        plan = run_case(bufs, case)
        if plan["active"]:
            live = [L for k, L in enumerate(plan["link"]) if k < plan["geom"].nparts and L["linked"]]
            assert live and all(L["serial"] == 1 for L in live), (case.name, plan["link"])


def test_representatives_through_the_one_wavefront_walk(bufs, stream_opts):
    """stream_rw 0 has no chunks: exact against the oracle, and the case is what it claims under the model"""
    W.set_option("stream_rw", 0)
    for case in representatives():
        bufs.run(case.wire, case.max_frames)
        fo, fl, res = S.frame_offsets(case.wire)
        g = S.geometry(case.wire, opts=case.opts, fo=fo, fl=fl)[0]
        for cell in case.cells:
            S.check_cell(cell, case.wire, case.max_frames, g, fo, fl, S.frame_offsets(case.wire, case.max_frames)[2])


def test_host_linked_walk_on_its_own_grid(bufs, stream_opts):
    """stream_rw 2: the geometry the host chose, read back, equals the model's (pass rounds, sample from
    where they stopped, the host rule), and chunk-start and window cells built on THAT grid hold under it;
    the representatives of the device grid are exact too"""
    W.set_option("stream_rw", 2)
    for case in S.host_cases() + representatives()[:4]:
        bufs.run(case.wire, case.max_frames)
        fo, fl, res = S.frame_offsets(case.wire)
        want = S.host_walk_geometry(case.wire, fo, fl)
        plan = read_plan()
        assert plan["path"] == 2 and want is not None and plan["active"] == 1, (case.name, plan)
        g, P1, nf, P = want
        t, u = plan["geom"].parts[0], g.parts[0]
        assert plan["geom"].nparts == 1 and plan["nf"] == nf, (case.name, plan)
        assert (t.P, t.C, t.H, t.n, t.capc, t.stgn) == (u.P, u.C, u.H, u.n, u.capc, u.stgn), (case.name, t, u)
        assert plan["link"][0]["nrows"] + plan["link"][0]["walks"] >= 1
        if case.name.startswith("host_"):
            for cell in case.cells:
                S.check_cell(cell, case.wire, case.max_frames, g, fo, fl, res)


def test_seen_max_carries_a_long_frame_into_the_next_window(bufs, stream_opts):
    """a 20 KiB frame outside the sample in call 1 gives call 2 windows of at least 24 KiB"""
    wire, fo, fl = S.base_stream()
    _, P1, ch = S.base_chunks()
    rng = np.random.default_rng(77)
    item = S._long_frame(rng, 20 * 1024)
    w1 = S.splice(wire, fo, [(ch[5][2] + 1000, item)], rng)
    run_case(bufs, S.Case("seen_call1", w1, S.BIG_MF, [("long", 5, 20 * 1024, False)], None))
    n0 = W.get_stat("stream_skips")
    bufs.run(wire, S.BIG_MF)
    assert W.get_stat("stream_skips") == n0 + 1
    plan = read_plan()
    g, _, _ = S.geometry(wire, seen=20 * 1024, fo=fo, fl=fl)
    assert plan["geom"] == g and g.parts[g.nparts - 1].H == 24 * 1024


def test_state_at_rest_after_each_kind_of_ending(bufs, stream_opts):
    """after a call that ended in the sample, in the passes, in part 0, at a hand-off and in the last chunk,
    the next call on the stream decodes a different stream exactly (and its plan is the model's)"""
    base, fo, fl = S.base_stream()
    other = S.cases("chunk_start")[1]
    uni, *_ = (np.frombuffer(S.uniform(np.random.default_rng(5), 3000, 40), dtype=np.uint8).copy(),)
    for k, v in S.THREE.items():
        W.set_option(k, v)
    g, P1, nf = S.geometry(base, opts=S.THREE, fo=fo, fl=fl)
    in1 = int(np.searchsorted(fo, g.parts[1].P))
    trunc = S.cases("stream_end")[-1]
    endings = [("sample", base, 100), ("passes", uni[:len(uni) - 3], S.BIG_MF), ("part 0", base, in1 - 50),
               ("hand-off", base, in1), ("last chunk", trunc.wire, S.BIG_MF)]
    for what, w, mf in endings:
        bufs.run(w, mf)
        bufs.run(other.wire, S.BIG_MF, shift=5)
        if what not in ("sample", "passes"):                   # (after those the hint is clear: the next call runs its rounds first)
            check_plan(S.Case(other.name, other.wire, S.BIG_MF, other.cells, None), 5, S.seen_after(w, mf), dict(S.THREE), what)


def _replay_set(dev, n, mf, wires, opts):
    """capture one call of length n and replay it on each stream in turn: every replay exact, bytes around the
    buffer and the guard after the descriptors untouched, the plan read back equal to the model's"""
    d = torch.zeros(16 + n + 64, dtype=torch.uint8, device=dev)
    desc = torch.zeros(mf * 32 + GUARD, dtype=torch.uint8, device=dev)
    res = torch.zeros(16, dtype=torch.uint8, device=dev)
    shift = 5
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        W.stream_decode_device(d[shift:], n, mf, desc, res)
    prev = None
    for i, case in enumerate(wires):
        w = case.wire
        host = np.concatenate([PAD[len(PAD) - shift:], w, PAD[:64]])
        d[:len(host)].copy_(torch.from_numpy(host))
        desc.fill_(0xEE)
        res.zero_()
        g.replay()
        torch.cuda.synchronize()
        ob = w.copy()
        od, orr = oracle_segments(ob, [0], [n], mf)
        gr = res.cpu().numpy().view(W.SEGRES_DTYPE)[0]
        assert tuple(gr) == tuple(orr[0]), (case.name, i)
        nf = int(gr["n_frames"])
        dh = desc.cpu().numpy()
        assert np.array_equal(dh[:nf * 32].view(W.DESC_DTYPE), od[:nf]), (case.name, i)
        assert (dh[mf * 32:] == 0xEE).all(), (case.name, i)
        got = d[:len(host)].cpu().numpy()
        assert np.array_equal(got[shift:shift + n], ob), (case.name, i)
        assert np.array_equal(got[:shift], host[:shift]) and np.array_equal(got[shift + n:], host[shift + n:]), (case.name, i)
        if prev is not None:                                  # (the first replay's hint and `seen` are the slot's past)
            check_plan(S.Case(case.name, w, mf, case.cells, None), shift, S.seen_after(prev.wire, mf), opts, "replay %d" % i)
        prev = case
    del g


def test_captured_replays_of_the_representatives(dev, stream_opts):
    """captured calls: one representative per cell group, each replayed twice, the second time after a replay
    of a different splice of the same length (it inherits that replay's hint and longest frame)"""
    base = S.Case("base", S.base_stream()[0], S.BIG_MF, [("split", "part0_empty")], None)
    a, b, c, e = S.cases("chunk_start")[1], S.cases("window_long")[2], S.cases("window_long")[7], S.cases("endings")[2]
    _replay_set(dev, S.BASE_BYTES, S.BIG_MF, [base, base, a, b, a, c, b, e, c, a, e], dict(S.DEFAULT_OPTS))
    cnt = S.cases("counts")[4]
    other = S.Case("start+0 cut", a.wire, cnt.max_frames, [], None)
    _replay_set(dev, S.BASE_BYTES, cnt.max_frames, [cnt, cnt, other, cnt], dict(S.DEFAULT_OPTS))
    end = S.cases("stream_end")[1]
    n = len(end.wire)
    _replay_set(dev, n, S.BIG_MF, [end, end, S.Case("cut", a.wire[:n].copy(), S.BIG_MF, [], None), end], dict(S.DEFAULT_OPTS))
    for k, v in S.THREE.items():
        W.set_option(k, v)
    h = S.cases("handoffs")[2]
    _replay_set(dev, S.BASE_BYTES, h.max_frames, [h, h, S.Case("o", a.wire, h.max_frames, [], dict(S.THREE)), h], dict(S.THREE))


def test_pass_loop_cases(dev, stream_opts):
    """the grid passes: pass A's 4096-candidate boundary, rounds running out, the 512 KiB threshold, g = 0.
    Every call here is meant for the pass rounds: the hint is cleared first and no call may skip them. After
    its rounds a stream of 512 KiB + 0 or + 1 has less than 512 KiB left, so one wavefront finishes it and the
    hint stays clear; those two then also run on the skip path on purpose (the hint set by the base stream),
    where the length alone decides and the chunk walk takes them"""
    small = Bufs(dev, S.BASE_BYTES, S.BIG_MF)
    base = S.base_stream()[0]
    clear_hint(small)
    try:
        for name, wire, mf, opts, claim in S.pass_cases():
            for k, v in opts.items():
                W.set_option(k, v)
            for shift in (0, 9):
                n0 = W.get_stat("stream_skips")
                small.run(wire, mf, shift)
                assert W.get_stat("stream_skips") == n0, (name, "skipped the pass rounds")
            W.set_option("stream_rounds", 4)
            if len(wire) >= M.MIN_STREAM:                      # 512 KiB + 0, + 1: the skip path too
                small.run(base, S.BIG_MF)
                small.run(base, S.BIG_MF)                      # (the hint is set now)
                n0 = W.get_stat("stream_skips")
                small.run(wire, mf)
                assert W.get_stat("stream_skips") == n0 + 1, (name, "not the skip path")
                assert W.get_stat("stream_plan_path") == 1 and W.get_stat("stream_plan_active") == 1, name
                clear_hint(small)
    finally:
        W.set_option("stream_rounds", 4)
    for name, wire, mf, active in S.rest_cases():               # a rest of 255 / 256 mean frames after the sample
        small.run(wire, mf)
        n0 = W.get_stat("stream_skips")
        small.run(wire, mf)
        assert W.get_stat("stream_skips") == n0 + 1, name
        plan = read_plan()
        assert plan["path"] == 1 and plan["active"] == active, (name, plan["active"])


def test_pass_b_second_grid_stride_step_and_the_plan_s_workspace_gone(dev):
    """one run of 6-byte frames longer than pass B's grid (8192 blocks of 256) plus pass A's 4096, decoded by
    the pass rounds (the hint cleared first, no skip). The call grows the stream's auxiliary workspace and
    plans no chunk walk, so the plan of the call before it lies in memory that is gone: the stats refuse"""
    wire, n = S.pass_b_case()
    # a stream no other test uses (none asks for a priority), so its workspace slot starts small
    big = Bufs(dev, len(wire), n + 10, stream=torch.cuda.Stream(dev, priority=-1))
    base = S.base_stream()[0]
    w0 = W.get_stat("workspace_bytes")
    big.run(base, S.BIG_MF)
    fresh = W.get_stat("workspace_bytes") > w0                  # (else the slot came with another stream's buffers)
    big.run(base, S.BIG_MF)
    assert W.get_stat("stream_plan_path") == 1 and W.get_stat("stream_plan_active") == 1
    clear_hint(big)
    assert W.get_stat("stream_plan_path") == 1                  # (smaller calls: the workspace stayed)
    n0, b0 = W.get_stat("stream_skips"), W.get_stat("workspace_bytes")
    r = big.run(wire, n + 10)
    assert W.get_stat("stream_skips") == n0, "the run was not decoded by the pass rounds"
    assert int(r["n_frames"]) == n and int(r["consumed"]) == len(wire)
    if fresh:
        assert W.get_stat("workspace_bytes") > b0
        for name in ("stream_plan_path", "stream_plan_nchunks", "stream_plan_C2"):
            with pytest.raises(ValueError):
                W.get_stat(name)
    else:                                                       # the workspace was large enough already: the plan still lies there
        assert W.get_stat("stream_plan_path") == 1
    big.run(base, S.BIG_MF)                                     # the next planned call is read back again
    big.run(base, S.BIG_MF)
    assert W.get_stat("stream_plan_path") == 1 and W.get_stat("stream_plan_active") == 1
