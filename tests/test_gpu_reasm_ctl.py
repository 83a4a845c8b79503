"""GPU parity of websocketframeBatchReassembleDeviceCtl with WEBSOCKET_REASM_CONTROL_DIRECT
(control frames delivered apart from fragmented messages, RFC 6455 5.4) against the reference's
own reactor under a control-direct glue (tests/golden/reassemble_ctl.json) and against the
rule's checker (tests/reasm_ctl_oracle.py, itself pinned to that fixture), bit-exact on both
kernel paths: descriptors, segment results, message descriptors in delivery order, data bodies
upward and control bodies downward in every region, untouched bytes everywhere else, open
state, cached bytes; the wire must come back untouched."""
import numpy as np
import pytest

import reasm_ctl_cases as R
from oracle_lib import oracle_reassemble, oracle_segments, used_descs
from reasm_ctl_oracle import oracle_reassemble_ctl, region_image
from test_gpu_parity import random_stream
from test_gpu_reasm import _frame, _segments
from util_amd import _lib
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CTL = W.REASM_CONTROL_DIRECT
FILL = 0xEE


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# reasm_path 1: fused one-workgroup-per-segment kernel, 2: scan + layout + gather kernels
@pytest.fixture(params=[1, 2], ids=["fused", "three_kernel"], autouse=True)
def reasm_path(request):
    W.set_option("reasm_path", request.param)
    yield request.param
    W.set_option("reasm_path", 0)


class Bufs:
    """device buffers of one call, outputs prefilled with 0xEE"""

    def __init__(self, dev, wire, so, sl, mf, open_in=None, out_off=None, out_size=None, cached_in=None, shift=0,
                 out_shift=0):
        n, nseg = len(wire), len(so)
        self.n, self.nseg, self.mf = n, nseg, mf
        self.d = torch.zeros(shift + n + 64, dtype=torch.uint8, device=dev)[shift:]    # base phases: slack + slice
        if n:
            self.d[:n] = torch.from_numpy(wire).to(dev)
        T = lambda a: torch.tensor(np.asarray(a, dtype=np.int64), device=dev)  # noqa: E731
        self.so, self.sl = T(so), T(sl)
        self.out_off = None if out_off is None else T(out_off)
        self.out = torch.full((out_shift + (out_size or n) + 64,), FILL, dtype=torch.uint8, device=dev)[out_shift:]
        assert (self.d.data_ptr() & 15, self.out.data_ptr() & 15) == (shift & 15, out_shift & 15)
        self.desc = torch.full((max(1, nseg * mf) * 32,), FILL, dtype=torch.uint8, device=dev)
        self.msg = torch.full((max(1, nseg * mf) * 32,), FILL, dtype=torch.uint8, device=dev)
        self.res = torch.zeros(max(1, nseg) * 16, dtype=torch.uint8, device=dev)
        self.nmsg = torch.zeros(max(1, nseg), dtype=torch.int32, device=dev)
        self.op = None if open_in is None else torch.tensor(np.asarray(open_in, dtype=np.uint8), device=dev)
        self.ca = None if cached_in is None else torch.tensor(np.asarray(cached_in, dtype=np.uint32).view(np.int32),
                                                              device=dev)

    def call(self, readcache_max=0, flags=CTL):
        W.batch_reassemble_device(self.d, self.so, self.sl, self.mf, self.desc, self.res, self.out, self.msg, self.nmsg,
                                  out_off=self.out_off, open_state=self.op, readcache_max=readcache_max, cached=self.ca,
                                  flags=flags)

    def host(self):
        torch.cuda.synchronize()
        return (self.out.cpu().numpy(), self.desc.cpu().numpy().view(W.DESC_DTYPE),
                self.res.cpu().numpy().view(W.SEGRES_DTYPE)[:self.nseg], self.msg.cpu().numpy().view(W.MSG_DTYPE),
                self.nmsg.cpu().numpy()[:self.nseg], None if self.op is None else self.op.cpu().numpy(),
                None if self.ca is None else self.ca.cpu().numpy().view(np.uint32))


def gpu_ctl(dev, wire, so, sl, mf, open_in=None, out_off=None, out_size=None, readcache_max=0, cached_in=None,
            flags=CTL, shift=0, out_shift=0):
    b = Bufs(dev, wire, so, sl, mf, open_in, out_off, out_size, cached_in, shift, out_shift)
    b.call(readcache_max, flags)
    h = b.host()
    assert np.array_equal(b.d[:len(wire)].cpu().numpy(), wire), "wire buffer modified"
    return h


def compare(got, oracle, so, sl, mf, out_off=None, tag=""):
    """a call's outputs against the checker's: every field, and every byte of the output buffer
    (data bodies, control bodies, 0xEE wherever nothing belongs)"""
    out, gd, gr, gm, gn, gop, gca = got
    od, orr, oms, oreg, oop, oca = oracle
    assert np.array_equal(gr, orr), tag
    assert np.array_equal(used_descs(gd, gr, mf), used_descs(od, orr, mf)), tag
    for s in range(len(so)):
        assert int(gn[s]) == len(oms[s]), (tag, s)
        for i, m in enumerate(oms[s]):
            g = gm[s * mf + i]
            assert tuple(int(g[f]) for f in W.MSG_DTYPE.names) == m, (tag, s, i)
    exp = np.full(len(out), FILL, np.uint8)
    for s in range(len(so)):
        ob = int(out_off[s]) if out_off is not None else int(so[s])
        exp[ob:ob + int(sl[s])] = region_image(oreg[s], sl[s], FILL)
    bad = np.flatnonzero(out != exp)
    assert len(bad) == 0, (tag, "first differing output byte", int(bad[0]) if len(bad) else None)
    if gop is not None:
        assert np.array_equal(gop, oop), tag
    if gca is not None:
        assert np.array_equal(gca, oca), tag


def check(dev, wire, so, sl, mf, open_in=None, out_off=None, out_size=None, readcache_max=0, cached_in=None, tag="",
          shift=0, out_shift=0, buflen=None, oracle=None):
    """shift / out_shift: the buffers' base phases; buflen: passed to the entry point as it is;
    oracle: oracle_reassemble_ctl's output for these arguments, where the caller has it already"""
    if buflen is None:
        got = gpu_ctl(dev, wire, so, sl, mf, open_in, out_off, out_size, readcache_max, cached_in, CTL, shift, out_shift)
    else:
        from test_gpu_reasm import gpu_reassemble
        got = gpu_reassemble(dev, wire, so, sl, mf, open_in, out_off, out_size, readcache_max, cached_in, shift,
                             out_shift, CTL, buflen)
    orc = oracle or oracle_reassemble_ctl(wire, so, sl, mf, open_in, out_off, readcache_max, cached_in)
    compare(got, orc, so, sl, mf, out_off, tag)
    return orc


def with_control(rng, wire, so, sl, share=0.2, lead=0.0):
    """rewrite the opcode of every frame the reactor loop reaches: a control one (8-15) for about
    `share` of them (and for a segment's first frames with probability `lead`), a data one (0-7)
    for the rest; FIN, RSV, lengths and masking stay as they are, so the framing is unchanged"""
    wire = wire.copy()
    desc, res = oracle_segments(wire.copy(), so, sl, 4096)
    for s in range(len(so)):
        leading = rng.random() < lead
        for k in range(int(res[s]["n_frames"])):
            a = int(desc[s * 4096 + k]["frame_off"])
            if a >= int(so[s]) + int(sl[s]):
                break
            leading = leading and rng.random() < 0.7
            if leading or rng.random() < share:
                wire[a] = (wire[a] & 0xF0) | int(rng.integers(8, 16))
            else:
                wire[a] = wire[a] & 0xF7
    return wire


# ------------------------------------------------------------------ the reference's own deliveries

def _gpu_reactor_view(dev, wire, max_frames, limit):
    """the stream decoded on the GPU batch after batch, d_open / d_cached carried across batches:
    the reference reactor's view of the whole stream (as test_gpu_reasm._gpu_reactor_view)"""
    pos, frames, lens, bodies = 0, 0, [], []
    op, ca = [0], [0]
    carry = np.zeros(0, np.uint8)
    while True:
        seg = wire[pos:]
        out, gd, gr, gm, gn, op, ca = gpu_ctl(dev, seg, [0], [len(seg)], max_frames, open_in=op, readcache_max=limit,
                                              cached_in=ca)
        for i in range(int(gn[0])):
            m = gm[i]
            part = out[int(m["out_off"]):int(m["out_off"]) + int(m["len"])]
            whole = np.concatenate([carry, part]) if int(m["continued"]) else part
            if int(m["complete"]):
                lens.append(len(whole))
                bodies.append(whole)
                if not int(gd[int(m["first_frame"])]["type"]) & 8:
                    carry = np.zeros(0, np.uint8)
            else:
                carry = whole
        st = int(gr[0]["status"])
        pos += int(gr[0]["consumed"])
        frames += int(gr[0]["n_frames"]) - (1 if st == -4 else 0)
        if st != 1:
            return (lens, np.concatenate(bodies) if bodies else np.zeros(0, np.uint8), pos, frames,
                    7 if st == -4 else 0, int(op[0]), int(ca[0]))


@pytest.mark.parametrize("mf", [16, 64, 0], ids=["mf16", "mf64", "whole"])
def test_ctl_reference_reactor_fixture(dev, golden, reasm_path, mf):
    """every stream of tests/golden/reassemble_ctl.json as one connection, in batches of at most
    mf frames (0: the whole stream as one segment, three-kernel path only): the GPU delivers
    exactly what the reference's reactor delivered under the control-direct glue"""
    if mf == 0 and reasm_path == 1:
        pytest.skip("fused path: max_frames <= 64")
    for c in golden("reassemble_ctl.json"):
        wire, limit = R.build(c["name"])
        assert R.sha256(wire) == c["wire_sha256"]
        lens, bodies, consumed, frames, det, pend, cached = _gpu_reactor_view(dev, wire, mf or c["frames"] + 2, limit)
        assert lens == c["msg_lens"], c["name"]
        assert R.sha256(bodies) == c["bodies_sha256"], c["name"]
        assert (consumed, frames, det, pend, cached) == (c["consumed"], c["frames"], c["detach_error"], c["pending"],
                                                         c["cached"]), c["name"]


# ------------------------------------------------------------------ the checker, many segments

@pytest.mark.parametrize("seed,mf", [(1, 16), (2, 4), (3, 1), (4, 64)])
def test_ctl_random_vs_oracle(dev, seed, mf):
    rng = np.random.default_rng(100 + seed)
    wire, so, sl = random_stream(rng, 1500)
    wire = with_control(rng, wire, so, sl)
    _, _, _, oreg, _, _ = check(dev, wire, so, sl, mf, tag="seed %d" % seed)
    assert sum(1 for r in oreg if len(r[1])) > 100 and sum(1 for r in oreg if len(r[2])) > 100


def test_ctl_out_regions_elsewhere(dev):
    """explicit output offsets (regions in a separate, larger buffer, in reverse order)"""
    rng = np.random.default_rng(122)
    wire, so, sl = random_stream(rng, 500)
    wire = with_control(rng, wire, so, sl)
    out_off = np.zeros(len(so), np.int64)
    o = 5
    for s in reversed(range(len(so))):
        out_off[s] = o
        o += int(sl[s]) + 3
    check(dev, wire, so, sl, 16, out_off=out_off, out_size=o + 16, tag="out_off")


def test_ctl_carry_open_state_leading_control(dev):
    """a random open state carried in, segments that start with control frames: they neither
    continue nor close the carried message"""
    rng = np.random.default_rng(121)
    wire, so, sl = random_stream(rng, 800)
    wire = with_control(rng, wire, so, sl, lead=0.6)
    open0 = rng.integers(0, 2, len(so)).astype(np.uint8)
    _, _, oms, _, _, _ = check(dev, wire, so, sl, 16, open_in=open0, tag="carry-in")
    assert any(ms and ms[0][5] == 0 and any(m[5] == 1 for m in ms[1:]) for ms in oms), "no control before a continued message"


def test_ctl_round_edges_max64(dev):
    """300 segments of up to 90 frames with 0-3 byte bodies, max_frames 64 (64 frames per walk
    round of the fused kernel, 16 per group of the layout kernel): control frames forced at round
    lanes 0 and 63, messages spanning the round boundary with control frames on both sides"""
    rng = np.random.default_rng(132)
    segs = []
    for i in range(300):
        n = int(rng.integers(0, 90))
        b0s = [(0x80 if rng.random() < 0.3 else 0) | (int(rng.integers(8, 16)) if rng.random() < 0.25 else int(rng.integers(0, 8)))
               for _ in range(n)]
        if i % 3 == 0:                    # control at lanes 0 and 63 of a round, data around them
            for k in (0, 63, 64):
                if k < n:
                    b0s[k] = 0x89
        if i % 3 == 1 and n > 70:         # one message over the boundary: ... data, ctl | ctl, data FIN
            for k, b in ((60, 0x02), (61, 0x00), (62, 0x09), (63, 0x8A), (64, 0x89), (65, 0x00), (66, 0x80)):
                b0s[k] = b
        segs.append([_frame(rng, int(rng.integers(0, 4)), masked=rng.random() < 0.8, b0=b) for b in b0s])
    wire, so, sl = _segments(segs, rng)
    check(dev, wire, so, sl, 64, tag="round edges")


def test_ctl_window_edges(dev):
    """data fragments and control bodies longer than the fused kernel's 20 KiB LDS window, headers
    straddling window edges, at every alignment"""
    rng = np.random.default_rng(131)
    segs = []
    for i in range(64):
        n = int(rng.integers(1, 8))
        parts = []
        for k in range(n):
            plen = int(rng.choice([20475, 20470, 20480, 40960 + 3, 70000, 0, 1]))
            ctl = rng.random() < 0.4
            b0 = (0x80 if (k == n - 1 or rng.random() < 0.3) else 0) | (int(rng.choice([8, 9, 10])) if ctl else (2 if k == 0 else 0))
            parts.append(_frame(rng, plen, masked=rng.random() < 0.9, b0=b0))
        segs.append(parts)
    wire, so, sl = _segments(segs, rng)
    check(dev, wire, so, sl, 16, tag="windows")


@pytest.mark.parametrize("limit", [1, 700, 4096])
def test_ctl_cache_limit_random_vs_oracle(dev, limit):
    """the fragment-cache limit over data frames only: control bodies are neither checked nor
    counted, so segments stop elsewhere than under the plain rule"""
    rng = np.random.default_rng(140 + limit)
    wire, so, sl = random_stream(rng, 1200)
    wire = with_control(rng, wire, so, sl)
    open0 = rng.integers(0, 2, len(so)).astype(np.uint8)
    cached0 = np.where(open0 == 1, rng.integers(0, 2 * limit, len(so)), 0).astype(np.uint32)
    _, orr, _, _, _, _ = oracle_reassemble_ctl(wire, so, sl, 16, open0, None, limit, cached0)
    assert (orr["status"] == -4).any(), "the limit never triggered: the case tests nothing"
    _, prr, _, _, _, _ = oracle_reassemble(wire, so, sl, 16, open0, None, limit, cached0)
    assert (prr["status"] != orr["status"]).any(), "no segment ends differently than with the flag off"
    check(dev, wire, so, sl, 16, open_in=open0, readcache_max=limit, cached_in=cached0, tag="limit %d" % limit)


# ------------------------------------------------------------------ the entry point itself

def test_ctl_flags_zero_is_the_plain_call(dev):
    """flags = 0 through the new entry, on a stream with control frames and a cache limit: every
    output byte equals websocketframeBatchReassembleDeviceEx's"""
    rng = np.random.default_rng(150)
    wire, so, sl = random_stream(rng, 600)
    wire = with_control(rng, wire, so, sl)
    open0 = rng.integers(0, 2, len(so)).astype(np.uint8)
    cached0 = np.where(open0 == 1, rng.integers(0, 3000, len(so)), 0).astype(np.uint32)
    lib, ctl_lib = W.load_lib(), _lib.load_ctl_lib()
    outs = []
    for entry in ("Ex", "Ctl"):
        b = Bufs(dev, wire, so, sl, 16, open0, None, None, cached0)
        args = [b.d.data_ptr(), b.d.numel() - W.BATCH_PAD, b.so.data_ptr(), b.sl.data_ptr(), b.nseg, 16, b.desc.data_ptr(),
                b.res.data_ptr(), b.out.data_ptr(), None, b.msg.data_ptr(), b.nmsg.data_ptr(), b.op.data_ptr(), 2000,
                b.ca.data_ptr()]
        st = torch.cuda.current_stream().cuda_stream
        if entry == "Ex":
            rc = lib.websocketframeBatchReassembleDeviceEx(*args, st)
        else:
            rc = ctl_lib.websocketframeBatchReassembleDeviceCtl(*args, 0, st)
        assert rc == 0
        outs.append(b.host())
    for x, y in zip(*outs):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    od, orr, oms, oreg, oop, oca = oracle_reassemble(wire, so, sl, 16, open0, None, 2000, cached0)
    compare(outs[1], (od, orr, oms, [(ob, body, body[:0]) for ob, body in oreg], oop, oca), so, sl, 16, tag="flags 0")


@pytest.mark.parametrize("flags", [2, 0x80000001])
def test_ctl_unknown_flag_is_refused(dev, flags):
    """an unknown flag bit: negative return, an error string, nothing launched"""
    rng = np.random.default_rng(151)
    wire, so, sl = random_stream(rng, 50)
    b = Bufs(dev, wire, so, sl, 16, [0] * len(so), None, None, [0] * len(so))
    lib = _lib.load_ctl_lib()
    rc = lib.websocketframeBatchReassembleDeviceCtl(
        b.d.data_ptr(), b.d.numel() - W.BATCH_PAD, b.so.data_ptr(), b.sl.data_ptr(), b.nseg, 16, b.desc.data_ptr(),
        b.res.data_ptr(), b.out.data_ptr(), None, b.msg.data_ptr(), b.nmsg.data_ptr(), b.op.data_ptr(), 0, b.ca.data_ptr(),
        flags, torch.cuda.current_stream().cuda_stream)
    assert rc < 0
    assert lib.websocketframeGpuLastError()
    out, gd, gr, gm, gn, gop, gca = b.host()
    assert (out == FILL).all() and (gd.view(np.uint8) == FILL).all() and (gm.view(np.uint8) == FILL).all()
    assert not gr.view(np.uint8).any() and not gn.any() and not gop.any() and not gca.any()
    with pytest.raises(RuntimeError):
        b.call(flags=flags)


def test_ctl_graph_replay(dev):
    """one captured call (the first call made before the capture) replayed twice over changed
    bytes, bit-exact both times"""
    rng = np.random.default_rng(160)
    wire, so, sl = random_stream(rng, 400)
    wires = [with_control(rng, wire, so, sl) for _ in range(2)]
    b = Bufs(dev, wires[0], so, sl, 16, [0] * len(so), None, None, [0] * len(so))
    b.call()                                                      # workspace exists from here
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.call()
    for w in (wires[1], wires[0]):
        b.d[:len(w)] = torch.from_numpy(w).to(dev)
        for t in (b.out, b.desc, b.msg):
            t.fill_(FILL)
        for t in (b.res, b.nmsg, b.op, b.ca):
            t.zero_()
        torch.cuda.synchronize()
        g.replay()
        compare(b.host(), oracle_reassemble_ctl(w, so, sl, 16, [0] * len(so), None, 0, [0] * len(so)), so, sl, 16,
                tag="replay")
