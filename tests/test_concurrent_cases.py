"""The jobs of tests/concurrent_cases.py before a GPU is involved: the expected outputs of every
directed-size job equal what the host twins return (send_host, control_replies_host,
proto_step_host folded over the frames, handshake_host, client_request_host, client_verify_host)
or, where there is no host twin (reassembly, encode, the text validator, the send-list mapper), the
oracle; the shapes within a kind are pairwise different; the hostile predecessors have the
properties claimed for them; the successors' workspaces are smaller than the predecessors' — in
bytes for send and reply, whose layouts tests/c/send_host.cpp and tests/c/reply_host.cpp export,
in slots and segments for the others (their layouts are not visible to the host). CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import concurrent_cases as CJ
import proto_oracle as P
import reply_oracle as R
import send_oracle as S
import text_oracle as T
from oracle_lib import oracle_encode_frames, oracle_segments
from util_amd import wsframe as W

HERE = os.path.dirname(os.path.abspath(__file__))


def exp(j, name, dtype=np.uint8, tail=CJ.TAIL):
    return j.outs[name][1][:-tail].view(dtype)


def directed(kind):
    return [CJ.jobs(kind)[0]] + (list(CJ.small(kind)) if kind in CJ._SMALL else [])


# ------------------------------------------------------------------ what section 1 promises

@pytest.mark.parametrize("kind", CJ.KINDS)
def test_shapes_differ_and_stay_small(kind):
    js = CJ.jobs(kind)
    assert len(js) >= 6 and len({j.shape for j in js}) == len(js)
    slots = sorted(j.slots for j in js)
    assert any(256 < n <= 256 + 8 for n in slots) and any(512 < n <= 512 + 8 for n in slots), slots
    assert any(900 <= j.nseg <= 1100 for j in js) and 10 <= js[0].nseg < 100
    for j in js + (list(CJ.hostile(kind)) + list(CJ.small(kind)) if kind in CJ._HOSTILE else []):
        assert j.slots <= CJ.MAX_SLOTS and j.wire_bytes <= CJ.MAX_WIRE, j.name
        for name, (init, e, m) in j.outs.items():
            assert len(init) == len(e) and (m is None or len(m) == len(e)), (j.name, name)
    if kind in ("send", "reply"):
        assert {j.par["role" if kind == "send" else "keyed"] for j in js} == {False, True}


def test_hostile_predecessors_are_what_they_claim():
    for j in CJ.hostile("proto"):
        r = exp(j, "pres", P.RES_DTYPE)
        assert (r["first_bad"] == 0).all() and (r["code"] == P.ERR_TOO_BIG).all() and (r["close_status"] == 1009).all()
        st = j.outs["state"][0][:-CJ.TAIL].view(np.uint64)
        assert (st & np.uint64(P.ST_OPEN)).all() and ((st & np.uint64(P.BYTES_MAX)) == j.par["limit"]).all()
    for j in CJ.hostile("reply"):
        r = exp(j, "rres", R.RES_DTYPE)
        assert (r["n_pong"] == j.mf - 1).all() and (r["close_kind"] == R.CLOSE_ECHO).all()
        per = (j.mf - 1) * (127 + 4 * j.par["keyed"]) + 4 + 4 * j.par["keyed"]
        assert (r["tx_len"] == per).all() and j.wire_bytes == per * j.nseg
        assert (j.ins["res"]["n_frames"] == j.mf).all()
    for j in CJ.hostile("text"):
        assert (j.ins["nmsg"] == j.mf).all() and not j.ins["msg"]["complete"].any()
        assert j.ins["msg"]["continued"].reshape(j.nseg, j.mf)[:, 0].all()
        st = exp(j, "state", np.uint32)
        assert (st & np.uint32(T.ST_PENDING)).all() and not (st & np.uint32(T.ST_FAILED)).any() and ((st >> 24) & 3).all()
        assert (exp(j, "verdict", np.uint32) == T.VALID).all()
    dense = [j for j in CJ.hostile("send") if j.wire_bytes]
    dead = [j for j in CJ.hostile("send") if not j.wire_bytes]
    assert {j.par["role"] for j in dense} == {j.par["role"] for j in dead} == {False, True}
    for j in dense:
        r = exp(j, "res", S.RES_DTYPE)
        assert (r["status"] == 0).all() and (r["n_msgs"] == j.mf).all() and (j.ins["nmsg"] == j.mf).all()
        F = 7 if j.par["role"] else 3
        assert (j.ins["frags"] == F).all() and S.shard_of(F, j.par["role"]) == 1 and not S.shard_of(F - 1, j.par["role"])
        assert (r["n_frames"] == j.ins["msg"]["len"].reshape(j.nseg, j.mf).sum(axis=1)).all()       # one body byte a frame
        assert j.wire_bytes > CJ.MAX_WIRE // 4
    for j in dead:
        r = exp(j, "res", S.RES_DTYPE)
        assert (r["status"] == S.ERR_FRAGMENT_SIZE).all() and (r["first_bad"] == 0).all() and not r["tx_len"].any()
    for j in CJ.hostile("reasm"):
        assert (exp(j, "res", W.SEGRES_DTYPE)["n_frames"] == j.mf).all()
        assert j.slots >= max(x.slots for x in CJ.jobs("reasm"))
    for j in CJ.hostile("encode"):
        assert j.nseg > max(x.nseg for x in CJ.jobs("encode"))


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """byte sizes of the send and reply workspaces, by the launchers' own formulas"""
    d = tmp_path_factory.mktemp("layouts")
    libs = {}
    for name in ("send", "reply"):
        so = str(d / ("lib%s_host.so" % name))
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "c", name + "_host.cpp"), "-o", so], check=True)
        libs[name] = C.CDLL(so)
    libs["send"].ws_send_host_layout.argtypes = [C.c_uint, C.c_uint, C.c_ulonglong, C.c_void_p]
    libs["reply"].ws_reply_host_layout.argtypes = [C.c_uint, C.c_uint, C.c_void_p]

    def size(j):
        out = np.zeros(10, np.uint64)
        if j.kind == "send":
            libs["send"].ws_send_host_layout(j.nseg, j.mf, j.par["cap"], out.ctypes.data)
        else:
            libs["reply"].ws_reply_host_layout(j.nseg, j.mf, out.ctypes.data)
        return int(out[6])
    return size


@pytest.mark.parametrize("kind", sorted(CJ._HOSTILE))
def test_successors_lie_inside_the_predecessors(kind, layouts):
    """fewer segments with a larger max_frames, and more segments with a smaller one; fewer slots
    either way, so every part of a successor's layout overlays a part the predecessor wrote"""
    a, b = CJ.small(kind)
    assert a.shape != b.shape
    for h in CJ.hostile(kind):
        for s in (a, b):
            assert s.slots < h.slots and s.nseg < h.nseg, (s.name, h.name)
            if kind in ("send", "reply"):
                assert layouts(s) < layouts(h), (s.name, h.name)
        if kind not in ("encode",):
            assert a.mf > h.mf > b.mf and a.nseg < b.nseg
        print(kind, "predecessor", h.name, h.shape, [layouts(h)] if kind in ("send", "reply") else "", "successors",
              [(s.shape, layouts(s) if kind in ("send", "reply") else None) for s in (a, b)])


# ------------------------------------------------------------------ the expectations are the host twins'

@pytest.mark.parametrize("j", directed("send"), ids=lambda j: j.name)
def test_send_expectations_equal_the_host_entry_point(j):
    tx, off, moff = exp(j, "tx", tail=4096), exp(j, "tx_off", np.uint64), exp(j, "moff", np.uint64)
    res = exp(j, "res", S.RES_DTYPE)
    for s in range(j.nseg):
        n = int(j.ins["nmsg"][s])
        keys = None if j.ins["keys"] is None else j.ins["keys"][s * j.mf:s * j.mf + n]
        total, got, gm, gr = W.send_host(j.ins["src"], j.ins["msg"][s * j.mf:s * j.mf + n], int(j.ins["frags"][s]), keys)
        assert total == int(off[s + 1] - off[s]) and got == bytes(tx[int(off[s]):int(off[s + 1])]), (j.name, s)
        assert gr == res[s] and [int(v) + int(off[s]) for v in gm] == [int(v) for v in moff[s * j.mf:s * j.mf + n]], (j.name, s)
        assert (moff[s * j.mf + n:(s + 1) * j.mf] == CJ.NONE64).all()


@pytest.mark.parametrize("j", directed("reply"), ids=lambda j: j.name)
def test_reply_expectations_equal_the_host_entry_point(j):
    tx, off, res = exp(j, "tx"), exp(j, "tx_off", np.uint64), exp(j, "rres", R.RES_DTYPE)
    i = j.ins
    for s in range(j.nseg):
        st = None if "state" not in j.outs else int(j.outs["state"][0].view(np.uint32)[s])
        n, got, rec, st_out = W.control_replies_host(
            i["buf"], i["seg_off"][s], i["desc"][s * j.mf:(s + 1) * j.mf], i["res"][s], j.mf, j.par["flags"],
            None if i["proto"] is None else i["proto"][s], 0 if i["fail"] is None else int(i["fail"][s]),
            None if i["keys"] is None else i["keys"][s * (j.mf + 1):(s + 1) * (j.mf + 1)], st)
        assert n == int(off[s + 1] - off[s]) and got == bytes(tx[int(off[s]):int(off[s + 1])]) and rec == res[s], (j.name, s)
        if st is not None:
            assert st_out == int(exp(j, "state", np.uint32)[s]), (j.name, s)


@pytest.mark.parametrize("j", directed("proto"), ids=lambda j: j.name)
def test_proto_expectations_equal_the_host_step_folded(j):
    i, mf = j.ins, j.mf
    wire, codes, res = i["buf"], exp(j, "codes"), exp(j, "pres", P.RES_DTYPE)
    for s in range(j.nseg):
        st = 0 if "state" not in j.outs else int(j.outs["state"][0].view(np.uint64)[s])
        was_closed = bool(st & P.ST_CLOSED)
        end = int(i["seg_off"][s]) + int(i["res"][s]["consumed"])
        first_bad, bad_code, close_frame = P.NONE, 0, P.NONE
        for k in range(min(int(i["res"][s]["n_frames"]), mf)):
            d = i["desc"][s * mf + k]
            ret, fo = int(d["ret"]), int(d["frame_off"])
            if not (ret > 0 and fo + ret <= end):
                assert codes[s * mf + k] == P.NOT_CONSUMED
                continue
            body2 = None
            if int(d["type"]) == 8 and int(d["datalen"]) >= 2:
                body2 = bytes(wire[int(d["data_off"]):int(d["data_off"]) + 2])
            if int(d["type"]) == 8 and not st & P.ST_CLOSED:
                close_frame = k
            code, st = W.proto_step_host(st, int(wire[fo]), int(d["masked"]), int(d["datalen"]), body2, j.par["flags"], j.par["rsv"],
                                         j.par["limit"])
            assert code == codes[s * mf + k], (j.name, s, k)
            if 1 <= code <= 10 and first_bad == P.NONE:
                first_bad, bad_code = k, code
        status = 0 if first_bad == P.NONE else (1009 if bad_code == P.ERR_TOO_BIG else 1002)
        assert tuple(int(v) for v in res[s]) == (first_bad, bad_code, status, P.NONE if was_closed else close_frame), (j.name, s)
        if "state" in j.outs:
            assert st == int(exp(j, "state", np.uint64)[s]), (j.name, s)


def test_handshake_expectations_equal_the_host_entry_point():
    j = CJ.jobs("handshake")[0]
    hs, acc, resp = exp(j, "hs", W.HS_DTYPE), exp(j, "acc").reshape(-1, 32), exp(j, "resp")
    cap = j.par["resp_cap"]
    for s, r in enumerate(j.reqs):
        d, a, text = W.handshake_host(r, j.par["flags"], cap)
        assert d == hs[s], (s, d, hs[s])
        assert bytes(acc[s]) == (a + b"\0\0\0\0" if a is not None else b"\x5a" * 32)
        want = resp[s * cap:(s + 1) * cap]
        n = 0 if text is None else len(text)
        assert bytes(want[:n]) == (text or b"") and (want[n:] == 0x77).all()


def test_client_request_expectations_equal_the_host_entry_point():
    j = CJ.jobs("client_request")[0]
    rd, req, expect = exp(j, "rd", W.CLI_REQ_DTYPE), exp(j, "req"), exp(j, "expect").reshape(-1, 32)
    cap = j.par["req_cap"]
    assert {int(f) for f in rd["flags"]} >= {W.CLI_REQ_WRITTEN, W.CLI_ERR_BYTES}
    for s, ((path, proto, host), nonce) in enumerate(zip(j.strings, j.nonces)):
        d, text, e = W.client_request_host(path, nonce, proto, host, cap)
        assert d == rd[s], (s, d, rd[s])
        assert bytes(expect[s]) == (e if e is not None else b"\x5a" * 32)
        want = req[s * cap:(s + 1) * cap]
        n = 0 if text is None else len(text)
        assert bytes(want[:n]) == (text or b"") and (want[n:] == 0x77).all()


def test_client_verify_expectations_equal_the_host_entry_point():
    j = CJ.jobs("client_verify")[0]
    cv = exp(j, "cv", W.CLI_VERIFY_DTYPE)
    for s, (d, o) in enumerate(j.cases):
        assert W.client_verify_host(d, CJ.CC.EXPECT, o, j.par["max_head"]) == cv[s], s
    assert {int(r) for r in cv["reason"]} == set(range(7))          # (TOO_LONG needs a max_head: the random jobs carry one)


# ------------------------------------------------------------------ ... or the oracle's

@pytest.mark.parametrize("j", directed("encode"), ids=lambda j: j.name)
def test_encode_expectations_equal_the_oracle(j):
    wire, offs = oracle_encode_frames(j.ins["src"], j.ins["frames"])
    assert bytes(exp(j, "dst", tail=4096)) == wire and np.array_equal(exp(j, "wire_off", np.uint64), offs)


@pytest.mark.parametrize("j", directed("reasm"), ids=lambda j: j.name)
def test_reassembly_and_send_list_expectations_follow_the_oracle(j):
    """every listed message's bytes are its frames' bodies from the decode oracle, in order; the
    send list names exactly the complete text and binary messages"""
    od, orr, oms, out, nmsg, msg = j.model
    lst = CJ.sendlist_expect(od, oms, j.nseg, j.mf).view(S.MSG_DTYPE)
    dec = j.ins["buf"].copy()
    oracle_segments(dec, j.ins["seg_off"], j.ins["seg_len"], j.mf)
    sent = 0
    for s in range(j.nseg):
        for i in range(int(nmsg[s])):
            m = msg[s * j.mf + i]
            fr = od[s * j.mf + int(m["first_frame"]):s * j.mf + int(m["first_frame"]) + int(m["n_frames"])]
            body = b"".join(bytes(dec[int(d["data_off"]):int(d["data_off"]) + int(d["datalen"])]) for d in fr if int(d["datalen"]))
            assert bytes(out[int(m["out_off"]):int(m["out_off"]) + int(m["len"])]) == body, (s, i)
            e = lst[s * j.mf + i]
            if m["complete"] and not m["continued"] and int(fr[0]["type"]) in (1, 2):
                assert (int(e["src_off"]), int(e["len"]), int(e["type"])) == (int(m["out_off"]), int(m["len"]), int(fr[0]["type"]))
                sent += 1
            else:
                assert int(e["type"]) == S.SKIP
        assert (lst[s * j.mf + int(nmsg[s]):(s + 1) * j.mf]["type"] == 0xEEEEEEEE).all()
    assert sent > 3


@pytest.mark.parametrize("j", directed("text"), ids=lambda j: j.name)
def test_text_expectations_equal_the_strict_decoder(j):
    """a text message that is not a continuation: VALID iff its bytes decode (complete) or are a
    prefix of bytes that do (open), by the literal definition"""
    v = exp(j, "verdict", np.uint32).reshape(j.nseg, j.mf)
    msg, desc, out = j.ins["msg"].reshape(j.nseg, j.mf), j.ins["desc"].reshape(j.nseg, j.mf), j.ins["out"]
    seen = set()
    for s in range(j.nseg):
        n = int(j.ins["nmsg"][s])
        assert (v[s, n:] == CJ.SENTINEL32).all()
        for i in range(n):
            m = msg[s, i]
            if m["continued"] or desc[s, i]["type"] != 1:
                continue
            body = bytes(out[int(m["out_off"]):int(m["out_off"]) + int(m["len"])])
            ok = T.complete_ok(body) if m["complete"] else T.viable_literal(body)
            assert v[s, i] == (T.VALID if ok else T.INVALID), (s, i, body)
            seen.add(int(v[s, i]))
    assert seen == {T.VALID, T.INVALID}
