"""Every device entry point besides the two decodes of tests/test_gpu_concurrent.py with other calls
in flight: several HIP streams at once, two host threads, more streams than the slot table of a
device holds, directly after a larger call of its own kind that left hostile bytes in the
workspace, and interleaved with the other workspace users on one stream. The jobs and their
expected outputs are tests/concurrent_cases.py's (checked against the host twins on the CPU by
tests/test_concurrent_cases.py). Every comparison is bit-exact and covers the sentinel bytes behind
every output and in every slot the call does not own; every input must come back unchanged.

The two invariants these tests pin ("Workspace slots"): every workspace part is written
before it is read within a call, and a slot is never shared by two streams' calls."""
import threading

import numpy as np
import pytest

import concurrent_cases as CJ
import proto_cases as PC
import proto_oracle as P
import reply_cases as RC
import send_oracle as S
import text_oracle as T
from oracle_lib import oracle_reassemble, used_descs
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TAIL = CJ.TAIL


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def up(dev, a):
    return torch.from_numpy(CJ.u8(a)).to(dev)


def i64(t):
    return t.view(torch.int64)


def i32(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------ one launcher per entry point

def l_send(t, o, j, st):
    n, cap = j.nseg, j.par["cap"]
    W.batch_send_device(t["src"], t["msg"], i32(t["nmsg"]), j.mf, o["tx"][:cap] if cap else None, o["tx_off"][:8 * (n + 1)],
                        o["res"][:32 * n], frag_size=t["frags"], mask_key=t["keys"], msg_tx_off=o["moff"][:8 * n * j.mf],
                        tx_capacity=cap, stream=st)


def l_reply(t, o, j, st):
    n = j.nseg
    W.batch_control_replies_device(t["buf"], i64(t["seg_off"]), t["desc"], t["res"], j.mf, o["tx"], o["tx_off"][:8 * (n + 1)],
                                   o["rres"][:16 * n], j.par["flags"], t["proto"], t["fail"], t["keys"],
                                   o["state"][:4 * n] if "state" in o else None, tx_capacity=j.par["cap"], stream=st)


def l_proto(t, o, j, st):
    n = j.nseg
    W.batch_check_protocol_device(t["buf"], i64(t["seg_off"]), t["desc"], t["res"], j.mf, o["pres"][:16 * n], j.par["flags"],
                                  j.par["rsv"], j.par["limit"], i64(o["state"][:8 * n]) if "state" in o else None,
                                  o["codes"][:n * j.mf], stream=st)


def l_text(t, o, j, st):
    n = j.nseg
    W.batch_validate_text_device(t["out"], t["desc"], t["msg"], i32(t["nmsg"]), j.mf, o["verdict"][:4 * n * j.mf],
                                 text_state=o["state"][:4 * n] if "state" in o else None, first_bad=o["first_bad"][:4 * n], stream=st)


def l_reasm(t, o, j, st):
    n = j.nseg
    W.batch_reassemble_device(t["buf"], i64(t["seg_off"]), i64(t["seg_len"]), j.mf, o["desc"][:-TAIL], o["res"][:16 * n], o["out"],
                              o["msg"][:-TAIL], i32(o["nmsg"][:4 * n]), stream=st)


def l_encode(t, o, j, st):
    cap = j.par["cap"]
    W.batch_encode_device(t["src"], t["frames"], o["dst"][:cap], i64(o["wire_off"][:8 * (j.nseg + 1)]), capacity=cap, stream=st)


def l_sendlist(t, o, j, st):
    W.batch_send_list_from_messages_device(t["desc"], t["msg"], i32(t["nmsg"]), j.mf, o["lst"][:-TAIL], stream=st)


def l_handshake(t, o, j, st):
    n = j.nseg
    W.batch_handshake_device(t["buf"], i64(t["seg_off"]), i64(t["seg_len"]), o["hs"][:32 * n], j.par["flags"], o["acc"][:32 * n],
                             o["resp"][:-TAIL], None, j.par["resp_cap"], stream=st)


def l_client_request(t, o, j, st):
    n = j.nseg
    W.batch_client_request_device(t["strs"], t["entry"], t["nonce"], o["req"][:-TAIL], o["expect"][:32 * n], o["rd"][:16 * n], None,
                                  j.par["req_cap"], stream=st)


def l_client_verify(t, o, j, st):
    W.batch_client_verify_device(t["buf"], i64(t["seg_off"]), i64(t["seg_len"]), t["expect"], o["cv"][:32 * j.nseg], t["strs"],
                                 t["entry"], j.par["max_head"], stream=st)


LAUNCH = dict(send=l_send, reply=l_reply, proto=l_proto, text=l_text, reasm=l_reasm, encode=l_encode, sendlist=l_sendlist,
              handshake=l_handshake, client_request=l_client_request, client_verify=l_client_verify)


class Run:
    """the device buffers of one job: inputs uploaded, outputs filled with their sentinels;
    launch() calls the library on a stream, check() holds every output against the job's"""

    def __init__(self, dev, job, stream=None):
        self.j, self.dev = job, dev
        self.t = {k: None if a is None else up(dev, a) for k, a in job.ins.items()}
        self.o = {k: up(dev, init) for k, (init, _e, _m) in job.outs.items()}
        self.stream = stream if stream is not None else torch.cuda.Stream(dev)
        self.ev = None

    def reset(self):
        for k, (init, _e, _m) in self.j.outs.items():
            self.o[k].copy_(up(self.dev, init))

    def launch(self, timed=False):
        if timed:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record(self.stream)
        LAUNCH[self.j.kind](self.t, self.o, self.j, self.stream)
        if timed:
            self.ev[1].record(self.stream)

    def check(self, tag=""):
        tag = "%s %s (%s)" % (tag, self.j.kind, self.j.name)
        for k, (_init, e, m) in self.j.outs.items():
            g = self.o[k].cpu().numpy()
            diff = g != e if m is None else (g != e) & m
            bad = np.flatnonzero(diff)
            assert not len(bad), "%s: %s byte %d of %d is %#x, expected %#x (%d differ)" % (
                tag, k, bad[0], len(e), g[bad[0]], e[bad[0]], len(bad))
        for k, a in self.j.ins.items():
            if a is not None:
                assert np.array_equal(self.t[k].cpu().numpy(), CJ.u8(a)), "%s: input %s modified" % (tag, k)


def largest_first(jobs):
    return sorted(jobs, key=lambda j: (j.wire_bytes, j.slots), reverse=True)


def overlapping_pairs(runs):
    """pairs of jobs whose [start event, end event] intervals on the device intersect"""
    base = runs[0].ev[0]
    iv = [(base.elapsed_time(r.ev[0]), base.elapsed_time(r.ev[1])) for r in runs]
    return sum(1 for a in range(len(iv)) for b in range(a + 1, len(iv)) if iv[a][0] < iv[b][1] and iv[b][0] < iv[a][1]), iv


# ------------------------------------------------------------------ the tests

@pytest.mark.parametrize("kind", CJ.KINDS)
def test_streams_in_flight(dev, kind):
    """six jobs of different layouts on six streams, launched back to back, largest first, with no
    host synchronisation between them. How many pairs of jobs overlapped on the device is printed,
    not asserted."""
    runs = [Run(dev, j) for j in largest_first(CJ.jobs(kind, 6))]
    torch.cuda.synchronize()
    for r in runs:
        r.launch(timed=True)
    torch.cuda.synchronize()
    pairs, iv = overlapping_pairs(runs)
    print("overlap %s: %d of 15 pairs; intervals (ms) %s" % (kind, pairs, ["%.3f-%.3f" % x for x in iv]))
    for i, r in enumerate(runs):
        r.check("stream %d" % i)


class Chain:
    """one connection batch through the whole rx-to-tx chain on one stream: decode (in place, on
    its own copy of the wire), reassemble (from the wire as received), validate text, check the
    protocol and build the control replies (from the decode's descriptors), map the messages to a
    send list, send. Expected values: the models, stage by stage."""

    def __init__(self, dev, nseg, mf, seed):
        rng = np.random.default_rng(seed)
        segs = []
        for s in range(nseg):
            fr = PC.quiet(int(rng.integers(0, mf + 1)), tail_open=rng.random() < 0.2)
            if fr and rng.random() < 0.3:
                fr[-1] = PC.close(1000 + s % 4)
            if fr and rng.random() < 0.1:
                fr[len(fr) // 2] = PC.frame(PC.TEXT, b"\xe2\x82", fin=1)          # not UTF-8; and, inside a message, interleaved
            segs.append(fr)
        self.b = b = PC.Batch(segs, mf, gap=3)
        self.nseg, self.mf, self.dev = nseg, mf, dev
        n, slots = nseg, nseg * mf
        so, sl = np.asarray(b.seg_off, np.uint64), np.asarray(b.seg_len, np.uint64)
        self.stream = torch.cuda.Stream(dev)
        full = lambda nbytes, v=CJ.FILL: torch.full((nbytes,), v, dtype=torch.uint8, device=dev)  # noqa: E731
        self.d_dec, self.d_raw, self.so, self.sl = up(dev, b.raw), up(dev, b.raw), i64(up(dev, so)), i64(up(dev, sl))
        self.desc1, self.res1 = full(32 * slots + TAIL), full(16 * n + TAIL)
        self.desc2, self.res2, self.msg, self.nmsg = full(32 * slots + TAIL), full(16 * n + TAIL), full(32 * slots + TAIL), full(4 * n + TAIL)
        self.out = full(len(b.raw) + 64)
        self.verdict, self.first_bad, self.tstate = full(4 * slots + TAIL, 0x5A), full(4 * n + TAIL, 0x5A), full(4 * n + TAIL, 0)
        self.codes, self.pres, self.pstate = full(slots + TAIL), full(16 * n + TAIL), full(8 * n + TAIL, 0)
        self.rstate = full(4 * n + TAIL, 0)
        self.lst = full(24 * slots + TAIL)
        # the models
        self.od, self.orr, self.oms, oreg, _, _ = oracle_reassemble(b.raw, b.seg_off, b.seg_len, mf)
        self.eout = np.full(len(b.raw) + 64, CJ.FILL, np.uint8)
        self.everdict = np.full(slots, CJ.SENTINEL32, np.uint32)
        self.efirst, self.etstate = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        conns = []
        for s in range(n):
            ob, body = oreg[s]
            self.eout[ob:ob + len(body)] = body
            ms = [(int(self.od[s * mf + first]["type"]), bytes(body[o - ob:o - ob + ln]), c, cont, nf)
                  for (o, ln, first, nf, c, cont) in self.oms[s]]
            v, self.efirst[s], self.etstate[s] = T.TextConn().batch(ms)
            self.everdict[s * mf:s * mf + len(v)] = v
        self.ecodes, self.epres, self.epstate = b.expect(P.EXPECT_MASKED, 0, 0, np.zeros(n, np.uint64))
        c = RC.Case(b, 0, None, None, None, np.zeros(n, np.uint32))
        c.proto = self.epres
        self.etx, self.etxoff, self.erres, self.erstate = c.expect()
        self.elst = CJ.sendlist_expect(self.od, self.oms, n, mf)
        rec = self.elst.view(S.MSG_DTYPE)
        for s in range(n):
            conns.append([(int(r["src_off"]), int(r["len"]), int(r["type"])) for r in rec[s * mf:s * mf + len(self.oms[s])]])
        self.estx, self.estxoff, self.esmoff, self.esres = S.batch(self.eout, conns, None, None, mf)
        self.tx, self.tx_off, self.rres = full(len(self.etx) + 256), full(8 * (n + 1) + TAIL), full(16 * n + TAIL)
        self.stx, self.stx_off, self.smoff, self.sres = full(len(self.estx) + 256), full(8 * (n + 1) + TAIL), full(8 * slots + TAIL), full(32 * n + TAIL)

    def launch(self):
        n, mf, st, slots = self.nseg, self.mf, self.stream, self.nseg * self.mf
        W.batch_decode_device(self.d_dec, self.so, self.sl, mf, self.desc1[:-TAIL], self.res1[:16 * n], stream=st)
        W.batch_reassemble_device(self.d_raw, self.so, self.sl, mf, self.desc2[:-TAIL], self.res2[:16 * n], self.out, self.msg[:-TAIL],
                                  i32(self.nmsg[:4 * n]), stream=st)
        W.batch_validate_text_device(self.out, self.desc2[:-TAIL], self.msg[:-TAIL], i32(self.nmsg[:4 * n]), mf, self.verdict[:4 * slots],
                                     text_state=self.tstate[:4 * n], first_bad=self.first_bad[:4 * n], stream=st)
        W.batch_check_protocol_device(self.d_dec, self.so, self.desc1[:-TAIL], self.res1[:16 * n], mf, self.pres[:16 * n],
                                      P.EXPECT_MASKED, 0, 0, i64(self.pstate[:8 * n]), self.codes[:slots], stream=st)
        W.batch_control_replies_device(self.d_dec, self.so, self.desc1[:-TAIL], self.res1[:16 * n], mf, self.tx, self.tx_off[:8 * (n + 1)],
                                       self.rres[:16 * n], 0, self.pres[:16 * n], None, None, self.rstate[:4 * n], stream=st)
        W.batch_send_list_from_messages_device(self.desc2[:-TAIL], self.msg[:-TAIL], i32(self.nmsg[:4 * n]), mf, self.lst[:-TAIL], stream=st)
        W.batch_send_device(self.out, self.lst[:-TAIL], i32(self.nmsg[:4 * n]), mf, self.stx, self.stx_off[:8 * (n + 1)], self.sres[:32 * n],
                            msg_tx_off=self.smoff[:8 * slots], stream=st)

    def check(self, tag):
        n, mf, b = self.nseg, self.mf, self.b
        host = lambda t: t.cpu().numpy()  # noqa: E731

        def same(name, t, want, fill=CJ.FILL):
            g, w = host(t), CJ.u8(want)
            bad = np.flatnonzero(g[:len(w)] != w)
            assert not len(bad), "%s: %s byte %d is %#x, expected %#x (%d differ)" % (tag, name, bad[0], g[bad[0]], w[bad[0]], len(bad))
            assert (g[len(w):] == fill).all(), "%s: bytes behind %s written" % (tag, name)
        same("decoded wire", self.d_dec, b.dec, 0x5A)
        same("wire as received", self.d_raw, b.raw, 0x5A)
        same("decode results", self.res1, b.res)
        gd = host(self.desc1)[:-TAIL].view(W.DESC_DTYPE)
        assert np.array_equal(used_descs(gd, b.res, mf), used_descs(b.desc, b.res, mf)), tag + ": decode descriptors"
        same("reassembly results", self.res2, self.orr)
        gd = host(self.desc2)[:-TAIL].view(W.DESC_DTYPE)
        assert np.array_equal(used_descs(gd, self.orr, mf), used_descs(self.od, self.orr, mf)), tag + ": reassembly descriptors"
        assert (host(self.desc1)[-TAIL:] == CJ.FILL).all() and (host(self.desc2)[-TAIL:] == CJ.FILL).all()
        same("message counts", self.nmsg, np.array([len(m) for m in self.oms], np.uint32))
        gm = host(self.msg)[:-TAIL].view(W.MSG_DTYPE)
        for s in range(n):
            for i, m in enumerate(self.oms[s]):
                assert tuple(int(gm[s * mf + i][f]) for f in W.MSG_DTYPE.names) == m, (tag, "message", s, i)
        same("bodies", self.out, self.eout)
        same("verdicts", self.verdict, self.everdict, 0x5A)
        same("text first_bad", self.first_bad, self.efirst, 0x5A)
        same("text state", self.tstate, self.etstate, 0)
        same("frame codes", self.codes, self.ecodes)
        same("protocol results", self.pres, self.epres)
        same("protocol state", self.pstate, self.epstate, 0)
        same("reply bytes", self.tx, np.frombuffer(self.etx, np.uint8))
        same("reply offsets", self.tx_off, self.etxoff)
        same("reply results", self.rres, self.erres)
        same("reply state", self.rstate, self.erstate, 0)
        same("send list", self.lst, self.elst)
        same("sent bytes", self.stx, self.estx)
        same("send offsets", self.stx_off, self.estxoff)
        same("message offsets", self.smoff, self.esmoff)
        same("send results", self.sres, self.esres)


def test_pipeline_per_stream(dev):
    """four streams, each running decode, reassemble, validate text, check protocol, control
    replies, send list from messages and send on its own batch with no host synchronisation inside
    or between the chains; the chains differ in segment count and max_frames"""
    chains = [Chain(dev, nseg, mf, 200 + i) for i, (nseg, mf) in enumerate(((40, 12), (300, 5), (9, 70), (129, 4)))]
    assert sum(len(c.etx) for c in chains) > 500 and sum(len(c.estx) for c in chains) > 1000
    assert any((c.everdict == T.INVALID).any() for c in chains) and any((c.epres["first_bad"] != P.NONE).any() for c in chains)
    torch.cuda.synchronize()
    for c in chains:
        c.launch()
    torch.cuda.synchronize()
    for i, c in enumerate(chains):
        c.check("chain %d" % i)


def test_two_host_threads(dev):
    """two jobs of each workspace-using kind, eight in all, split alternately over two host threads,
    each job on its own stream"""
    runs = [Run(dev, j) for kind in CJ.WS_KINDS for j in (CJ.jobs(kind)[3], CJ.jobs(kind)[1])]
    torch.cuda.synchronize()
    errs = []

    def work(part):
        try:
            torch.cuda.set_device(dev)
            for r in part:
                r.launch()
        except Exception as e:                     # noqa: BLE001 (reported below)
            errs.append(e)

    ts = [threading.Thread(target=work, args=(runs[k::2],)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    torch.cuda.synchronize()
    assert not errs, errs
    for i, r in enumerate(runs):
        r.check("thread job %d" % i)


@pytest.mark.parametrize("kind", CJ.WS_KINDS)
def test_more_streams_than_slots(dev, kind):
    """20 streams > the 16 eager workspace slots of a device, in the library the wrapper of this
    kind loads (each library keeps a slot table of its own): twice round, the outputs filled with
    their sentinels again between the rounds, every result exact in both"""
    js = CJ.jobs(kind, 5)
    runs = [Run(dev, js[i % 5]) for i in range(20)]
    torch.cuda.synchronize()
    for rnd in range(2):
        for r in runs:
            r.launch()
        torch.cuda.synchronize()
        for i, r in enumerate(runs):
            r.check("round %d slot job %d" % (rnd, i))
            r.reset()
        torch.cuda.synchronize()


@pytest.mark.parametrize("kind", sorted(CJ._HOSTILE))
def test_hostile_predecessor_then_small(dev, kind):
    """On one fresh stream, with no host synchronisation: a small job, the hostile predecessors of
    its kind, the small job again into fresh output buffers, a second small job of another layout.
    All calls' outputs are exact; the first small call's outputs must survive the workspace growth
    the predecessor causes (the library drains the stream before it frees the old buffer, so they
    are final by then). A fresh stream's slot is new, or an older stream's smaller one, so the
    growth is provoked by the order of the calls; the test cannot observe it and does not assert it."""
    a, b = CJ.small(kind)
    stream = torch.cuda.Stream(dev)
    runs = [Run(dev, j, stream) for j in (a,) + tuple(CJ.hostile(kind)) + (a, b)]
    torch.cuda.synchronize()
    for r in runs:
        r.launch()
    torch.cuda.synchronize()
    for i, r in enumerate(runs):
        r.check("call %d" % i)


def test_same_stream_two_kinds_interleaved(dev):
    """proto, reply, text and send calls in turn on one stream, three rounds with changing shapes,
    no synchronisation: each kind finds only its own buffer kind's previous contents"""
    stream = torch.cuda.Stream(dev)
    runs = [Run(dev, CJ.jobs(kind)[(2 * rnd + k) % 6], stream) for rnd in range(3) for k, kind in enumerate(("proto", "reply", "text", "send"))]
    torch.cuda.synchronize()
    for r in runs:
        r.launch()
    torch.cuda.synchronize()
    for i, r in enumerate(runs):
        r.check("call %d" % i)


def test_handshake_and_client_calls_beside_workspace_users(dev):
    """the three calls that take no workspace on three streams, a send and a reply call in flight on
    two more"""
    runs = [Run(dev, CJ.jobs(kind)[3]) for kind in ("send", "reply", "handshake", "client_request", "client_verify")]
    torch.cuda.synchronize()
    for r in runs:
        r.launch()
    torch.cuda.synchronize()
    for i, r in enumerate(runs):
        r.check("stream %d" % i)
