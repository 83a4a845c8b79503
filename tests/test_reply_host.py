"""The control replies' rule (util_amd/csrc/ws_reply.h: a frame's contribution, the run summary
and its combine, the segment's plan, the frame writer, the workspace layout) compiled for the host
and held against the sequential model (reply_oracle.py) and the hand-written table
(reply_cases.py); the exported host entry point against the same; the reply streams through the
oracle's reference decoder; the stand-alone sanitizer build; the symbol table of
libwsframe_amd_reply.so. CPU only: g++, ctypes and numpy."""
import ctypes as C
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import proto_cases as PC
import proto_oracle as P
import reply_cases as RC
import reply_oracle as R
from oracle_lib import load_oracle, oracle_segments
from test_abi import dynamic_symbols
from util_amd import _lib
from util_amd import wsframe as W

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "reply_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("reply") / "libreply_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so_path], check=True)
    lib = C.CDLL(so_path)
    vp, u32, u64 = C.c_void_p, C.c_uint, C.c_ulonglong
    lib.ws_reply_host_segment.restype = C.c_longlong
    lib.ws_reply_host_segment.argtypes = [vp, u64, vp, vp, u32, u32, vp, u32, vp, vp, vp, u64, vp]
    lib.ws_reply_host_runs.restype = C.c_longlong
    lib.ws_reply_host_runs.argtypes = [vp, u64, vp, vp, u32, u32, vp, u32, vp, vp, vp, u64, vp, vp, u32]
    lib.ws_reply_host_assoc.restype = u32
    lib.ws_reply_host_assoc.argtypes = [vp, u32, u32, u32, u32, u32]
    lib.ws_reply_host_layout.restype = None
    lib.ws_reply_host_layout.argtypes = [u32, u32, vp]
    lib.ws_reply_host_sizes.restype = u32
    return lib


def run_segment(fn, c, s, cuts=None, cap=None, flags=None, state="own"):
    """segment s of Case c through one of the C entry points (fn: the driver's sequential routine,
    its run form with `cuts`, or the exported host entry point). Returns (length, reply bytes that
    fit, result tuple, state out or None, the bytes past the reply: all FILL)."""
    b = c.b
    mf = b.max_frames
    flags = c.flags if flags is None else flags
    wire = c.wire(flags)
    desc = np.ascontiguousarray(b.desc[s * mf:(s + 1) * mf])
    res = np.ascontiguousarray(b.res[s:s + 1])
    pr = None if c.proto is None else np.ascontiguousarray(c.proto[s:s + 1])
    keys = None if c.keys is None else np.ascontiguousarray(c.keys[s * (mf + 1):(s + 1) * (mf + 1)])
    cap = 131 * mf + 8 if cap is None else cap
    tx = np.full(cap + 16, R.FILL, np.uint8)
    out = np.zeros(1, R.RES_DTYPE)
    st_in = c.state if isinstance(state, str) else state
    st = None if st_in is None else C.c_uint(int(st_in[s]))
    args = [wire.ctypes.data, int(b.seg_off[s]), desc.ctypes.data, res.ctypes.data, mf, flags,
            None if pr is None else pr.ctypes.data, 0 if c.fail is None else int(c.fail[s]),
            None if keys is None else keys.ctypes.data, None if st is None else C.addressof(st), tx.ctypes.data, cap,
            out.ctypes.data]
    if cuts is not None:
        ca = np.asarray(cuts, np.uint32)
        args += [ca.ctypes.data, len(ca)]
    n = fn(*args)
    fit = min(max(n, 0), cap)
    return n, bytes(tx[:fit]), tuple(int(v) for v in out[0]), None if st is None else st.value, tx[fit:]


def check_segment(got, exp, s, tag):
    """got: run_segment's answer; exp: (tx, tx_off, res, state) of the whole batch"""
    n, tx, res, st, rest = got
    etx, eoff, eres, est = exp
    lo, hi = int(eoff[s]), int(eoff[s + 1])
    assert n == hi - lo and tx == etx[lo:lo + len(tx)], "%s segment %d: %d bytes %s, expected %s" % (
        tag, s, n, tx.hex(), etx[lo:hi].hex())
    assert res == tuple(int(v) for v in eres[s]), "%s segment %d: result %s, expected %s" % (tag, s, res, eres[s])
    assert st == (None if est is None else int(est[s])), "%s segment %d: state" % (tag, s)
    assert (rest == R.FILL).all(), "%s segment %d: bytes past the reply written" % (tag, s)


# ------------------------------------------------------------------ 1: driver vs model and table

@pytest.mark.parametrize("wm", [0, R.WIRE_MASKED])
def test_table_literals_are_what_the_model_says(wm):
    for rows in RC.table_groups():
        c = RC.table_case(rows, wm)
        etx, eoff, eres, est = RC.table_expect(rows)
        mtx, moff, mres, mst = c.expect()
        for s, r in enumerate(rows):
            assert mtx[int(moff[s]):int(moff[s + 1])] == r["tx"], r["name"]
            assert tuple(mres[s]) == r["res"], r["name"]
        assert np.array_equal(moff, eoff) and (est is None) == (mst is None)
        assert est is None or np.array_equal(mst, est)


@pytest.mark.parametrize("wm", [0, R.WIRE_MASKED])
def test_driver_and_entry_point_give_the_table(host, wm):
    entry = _lib.load_reply_lib().websocketframeControlRepliesHost
    for rows in RC.table_groups():
        c = RC.table_case(rows, wm)
        exp = RC.table_expect(rows)
        for s, r in enumerate(rows):
            for fn, name in ((host.ws_reply_host_segment, "header"), (entry, "entry point")):
                check_segment(run_segment(fn, c, s), exp, s, "%s, %s" % (name, r["name"]))


def test_random_cases_cover_the_rule():
    seen = RC.coverage(RC.random_cases())
    assert seen["kinds"] == {0, 1, 2, 3} and seen["roles"] == {False, True}
    assert seen["wire_masked"] == {False, True} and seen["last"] == {False, True}
    assert seen["empty"] >= 10 and seen["carried"] >= 10 and seen["silenced"] >= 5 and seen["pongs"] >= 300, seen


def test_driver_and_entry_point_match_the_model_on_random_batches(host):
    entry = _lib.load_reply_lib().websocketframeControlRepliesHost
    rng = np.random.default_rng(7)
    for i, c in enumerate(RC.random_cases()):
        exp = c.expect()
        for s in range(c.b.nseg):
            n = int(c.b.res[s]["n_frames"])
            check_segment(run_segment(host.ws_reply_host_segment, c, s), exp, s, "header, batch %d" % i)
            check_segment(run_segment(entry, c, s), exp, s, "entry point, batch %d" % i)
            cuts = sorted(int(v) for v in rng.integers(0, n + 2, int(rng.integers(0, 4))))
            check_segment(run_segment(host.ws_reply_host_runs, c, s, cuts=cuts), exp, s, "runs %s, batch %d" % (cuts, i))
        alone = c.expect(state=None)
        for s in range(0, c.b.nseg, 5):
            check_segment(run_segment(entry, c, s, state=None), alone, s, "entry point, no state, batch %d" % i)


def test_capacity_cuts(host):
    """every capacity from 0 to the reply's length + 1 on the table's longest rows: the length
    and the result do not change, no byte at or past the capacity is written"""
    for rows in RC.table_groups():
        c = RC.table_case(rows)
        exp = RC.table_expect(rows)
        for s, r in enumerate(rows):
            if not 0 < len(r["tx"]) <= 16 and "125" not in r["name"]:
                continue
            for cap in range(len(r["tx"]) + 2):
                check_segment(run_segment(host.ws_reply_host_segment, c, s, cap=cap), exp, s, "cap %d, %s" % (cap, r["name"]))
                check_segment(run_segment(host.ws_reply_host_runs, c, s, cuts=[1], cap=cap), exp, s,
                              "runs, cap %d, %s" % (cap, r["name"]))


# ------------------------------------------------------------------ 2: the combine is associative

def script():
    """fourteen frames: pings of several lengths, one too long, one without FIN, data, a CLOSE,
    frames after it"""
    f, p = PC.frame, PC.PING
    return [f(p, b"a"), f(PC.TEXT, b"t", fin=0), f(p, b"bcd"), f(PC.CONT, b"u"), f(p, b"x" * 126), f(p, b"e" * 125),
            f(p, b"f", fin=0), f(PC.PONG, b"g"), f(p), f(p, b"hi"), PC.close(1001, b"bye"), f(p, b"late"), PC.close(1000),
            f(PC.BIN, b"z")]


@pytest.mark.parametrize("flags", [0, R.LAST_PING_ONLY, R.WIRE_MASKED, R.WIRE_MASKED | R.LAST_PING_ONLY])
@pytest.mark.parametrize("keyed", [False, True])
def test_every_split_into_two_and_three_runs(host, flags, keyed):
    """the script folded from every split into 2 and 3 runs equals the sequential result, with
    first_bad nowhere, before the CLOSE, on it and after it"""
    frames = script()
    n = len(frames)
    b = PC.Batch([frames], n + 1)
    keys = np.arange(1, n + 3, dtype=np.uint32) * 0x01020408 if keyed else None
    for fb in (R.NONE, 0, 3, 9, 10, 12):
        c = RC.Case(b, flags, [(fb, 1002)], None, keys, np.zeros(1, np.uint32))
        exp = c.expect()
        check_segment(run_segment(host.ws_reply_host_segment, c, 0), exp, 0, "sequential, first_bad %d" % fb)
        for a in range(n + 1):
            check_segment(run_segment(host.ws_reply_host_runs, c, 0, cuts=[a]), exp, 0, "cut %d first_bad %d" % (a, fb))
            for d in range(a, n + 1):
                check_segment(run_segment(host.ws_reply_host_runs, c, 0, cuts=[a, d]), exp, 0,
                              "cuts %d,%d first_bad %d" % (a, d, fb))


def test_combine_is_associative_on_random_runs(host):
    """(a op b) op c == a op (b op c) for 20,000 random triples of runs of 0..4 frames"""
    rng = np.random.default_rng(65)
    kinds = [(9, 1, 0), (9, 1, 5), (9, 1, 125), (9, 1, 126), (9, 0, 1), (8, 1, 2), (8, 1, 0), (1, 1, 3), (10, 1, 1)]
    for _ in range(20000):
        na, nb, nc = (int(v) for v in rng.integers(0, 5, 3))
        f = np.array([kinds[int(i)] for i in rng.integers(0, len(kinds), na + nb + nc)] or [(0, 0, 0)], np.uint32)
        fb = int(rng.choice([R.NONE, 0, 1, 3, 6, 20]))
        assert host.ws_reply_host_assoc(f.ctypes.data, na, nb, nc, fb, int(rng.integers(0, 2))) == 0, (f, na, nb, nc, fb)


# ------------------------------------------------------------------ 3: through the reference decoder

def decode_stream(tx):
    """the reply bytes as one segment through the oracle's decoder: [(type, is_fin, plain body)]"""
    buf = np.frombuffer(tx + b"\0" * PC.PAD, np.uint8).copy()
    desc, res = oracle_segments(buf, [0], [len(tx)], 4096)
    assert int(res[0]["consumed"]) == len(tx) and int(res[0]["status"]) == 0
    out = []
    for d in desc[:int(res[0]["n_frames"])]:
        n = int(d["datalen"])
        out.append((int(d["type"]), int(d["is_fin"]), bytes(buf[int(d["data_off"]):int(d["data_off"]) + n]) if n else b""))
    return out


def test_reply_streams_decode_to_the_expected_frames(host):
    """every reply the header emits, table and random, server and client role, is a stream of
    frames the reference decoder takes apart into exactly the model's (type, is_fin, body) list;
    the first two bytes of every frame are the reference encoder's (plus the MASK bit for a key)"""
    enc = load_oracle()
    cases = [RC.table_case(rows, wm) for rows in RC.table_groups() for wm in (0, R.WIRE_MASKED)] + RC.random_cases()
    frames_seen = 0
    for c in cases:
        b = c.b
        mf = b.max_frames
        for s in range(b.nseg):
            _n, tx, _res, _st, _rest = run_segment(host.ws_reply_host_segment, c, s)
            _, _, _, sent = R.segment(c.wire(), b.seg_off[s], b.desc[s * mf:(s + 1) * mf], b.res[s], mf, c.flags,
                                      None if c.proto is None else (c.proto[s]["first_bad"], c.proto[s]["close_status"]),
                                      0 if c.fail is None else int(c.fail[s]),
                                      None if c.keys is None else c.keys[s * (mf + 1):(s + 1) * (mf + 1)],
                                      0 if c.state is None else int(c.state[s]))
            got = decode_stream(tx)
            assert got == sent, (s, tx.hex())
            pos = 0
            for typ, fin, body in sent:
                h = (C.c_ubyte * 10)()
                enc.ws_oracle_encode(h, 1, 1, typ, len(body))
                assert enc.ws_oracle_encode_headlen(len(body)) == 2
                assert (tx[pos], tx[pos + 1] & 0x7F, tx[pos + 1] >> 7) == (h[0], h[1], int(c.keys is not None))
                pos += 2 + (4 if c.keys is not None else 0) + len(body)
                frames_seen += 1
    assert frames_seen >= 500


# ------------------------------------------------------------------ 4: the stand-alone program

def case_file(path):
    """the directed table, one case per row, in the format tests/c/reply_host.cpp reads"""
    blobs = []
    for rows in RC.table_groups():
        for wm in (0, R.WIRE_MASKED):
            c = RC.table_case(rows, wm)
            b = c.b
            mf = b.max_frames
            for s, r in enumerate(rows):
                wire = c.wire()
                st = 0xFFFFFFFF if r["state"] is None else r["state"]
                head = struct.pack("<15IQ", len(wire), mf, c.flags, 1, int(c.proto[s]["first_bad"]),
                                   int(c.proto[s]["close_status"]), r["fail"], int(r["keyed"]), st, len(r["tx"]), *r["res"],
                                   0 if r["state_out"] is None else r["state_out"], b.seg_off[s])
                keys = c.keys[s * (mf + 1):(s + 1) * (mf + 1)].tobytes() if r["keyed"] else b""
                blobs.append(head + wire.tobytes() + b.desc[s * mf:(s + 1) * mf].tobytes() + b.res[s:s + 1].tobytes() + keys +
                             r["tx"])
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blobs)) + b"".join(blobs))
    return len(blobs)


def test_host_program_under_sanitizers(tmp_path):
    """the same source as a program of its own, built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as its own process: the table under every capacity (the
    reply buffer is exactly that long) and every cut into two runs, the 125- and 126-byte pings
    among its rows"""
    exe = str(tmp_path / "reply_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DREPLY_HOST_MAIN", SRC, "-o", exe], check=True)
    ncase = case_file(str(tmp_path / "table.bin"))
    names = [r["name"] for r in RC.directed_table()]
    assert any("125" in n for n in names) and any("126" in n for n in names)
    out = subprocess.run([exe, str(tmp_path / "table.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("reply_host ok: %d cases" % ncase), out.stdout + out.stderr


# ------------------------------------------------------------------ layout, ABI, arguments

def up(x, a):
    return (x + a - 1) // a * a


@pytest.mark.parametrize("nseg,mf", [(1, 1), (3, 7), (255, 2), (256, 1), (257, 300), (1000, 301), (65536, 16), (1 << 20, 1),
                                      (1, 1 << 20), (1 << 15, 1 << 15)])
def test_workspace_layout(host, nseg, mf):
    """ws_reply.h's layout against the formulas written out here: regions in order, 16-B aligned,
    none overlapping, the sizes the kernels index"""
    assert host.ws_reply_host_sizes() == 32 | 32 << 8 | 16 << 16
    got = np.zeros(9, np.uint64)
    host.ws_reply_host_layout(nseg, mf, got.ctypes.data)
    nb, nt = (nseg + 255) // 256, (nseg * mf + 255) // 256
    bo = 16
    loff = bo + up(4 * (nb + 1), 16)
    bo64 = loff + 4 * 256 * nb
    rec = bo64 + up(8 * (nb + 1), 16)
    tail = rec + 32 * nseg
    agg = tail + 32 * nseg
    assert [int(v) for v in got] == [bo, loff, bo64, rec, tail, agg, agg + 32 * nt, nb, nt]
    assert all(int(v) % 16 == 0 for v in got[:7])


def test_reply_library_exports():
    """libwsframe_amd_reply.so's symbol table is libwsframe_amd_hs.so's plus exactly the names
    wsframe_amd_reply.h marks; the older libraries export none of them"""
    src = open(os.path.join(_lib.REPO, "include", "wsframe_amd_reply.h")).read()
    marked = set(re.findall(r"WSFRAME_AMD_REPLY_EXPORT[^;]*?\b(websocketframe\w+)\s*\(", src, re.S))
    assert marked == set(_lib.REPLY_EXPORTS) and len(marked) == 2
    assert os.path.exists(_lib.REPLY_LIB_PATH), "libwsframe_amd_reply.so is not built"
    assert dynamic_symbols(_lib.REPLY_LIB_PATH) == dynamic_symbols(_lib.HS_LIB_PATH) | marked
    for path in (_lib.LIB_PATH, _lib.CTL_LIB_PATH, _lib.TEXT_LIB_PATH, _lib.PROTO_LIB_PATH, _lib.HS_LIB_PATH,
                 _lib.BENCH_LIB_PATH):
        assert not dynamic_symbols(path) & marked, path


def test_constants_agree(tmp_path):
    """the header's values, wsframe.py's and the model's; the struct is 16 bytes; WIRE_MASKED is
    the protocol check's"""
    src = open(os.path.join(_lib.REPO, "include", "wsframe_amd_reply.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"WEBSOCKET_REPLY_(CLOSE_\w+) = (\d+)", src)}
    assert len(enum) == 4
    for name, value in enum.items():
        assert getattr(W, "REPLY_" + name) == value == getattr(R, name), name
    defs = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define WEBSOCKET_REPLY_(\w+)\s+(\w+)", src)}
    assert defs == {"WIRE_MASKED": 4, "LAST_PING_ONLY": 8, "NONE": 0xFFFFFFFF, "ST_CLOSE_SENT": 1}
    for name, value in defs.items():
        assert getattr(W, "REPLY_" + name) == value == getattr(R, name), name
    assert W.REPLY_WIRE_MASKED == W.PROTO_WIRE_MASKED == P.WIRE_MASKED
    assert W.REPLY_RES_DTYPE == R.RES_DTYPE and R.RES_DTYPE.itemsize == 16
    prog = tmp_path / "size.c"
    prog.write_text('#include "wsframe_amd_reply.h"\n#include <stdio.h>\nint main(void) { printf("%zu %u %u", '
                    "sizeof(WebsocketReplyResult_t), WEBSOCKET_REPLY_WIRE_MASKED, WEBSOCKET_PROTO_WIRE_MASKED); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(_lib.REPO, "include"), str(prog), "-o", exe],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "16 4 4"


def test_entry_point_refuses_bad_arguments():
    lib = _lib.load_reply_lib()
    c = RC.table_case(RC.table_groups()[0])
    mf = c.b.max_frames
    desc, res = np.ascontiguousarray(c.b.desc[:mf]), np.ascontiguousarray(c.b.res[:1])
    tx = np.full(64, R.FILL, np.uint8)
    out = np.full(4, 7, np.uint32)
    st = C.c_uint(0)

    def call(buf=c.b.dec.ctypes.data, d=desc.ctypes.data, r=res.ctypes.data, m=mf, flags=0, t=tx.ctypes.data, cap=64,
             o=out.ctypes.data):
        return lib.websocketframeControlRepliesHost(buf, int(c.b.seg_off[0]), d, r, m, flags, None, 0, None, C.addressof(st), t,
                                                    cap, o)
    for kw, word in ((dict(flags=1), b"flag"), (dict(flags=16), b"flag"), (dict(m=0), b"max_frames"), (dict(buf=None), b"NULL"),
                     (dict(d=None), b"NULL"), (dict(r=None), b"NULL"), (dict(o=None), b"NULL"), (dict(t=None), b"NULL")):
        assert call(**kw) < 0 and word in lib.websocketframeGpuLastError(), kw
        assert (tx == R.FILL).all() and (out == 7).all() and st.value == 0
    assert call(t=None, cap=0) == 2 and tuple(out) == (1, 0, 0, 2)          # "ping empty": the length without a buffer
    n, got, rec, state = W.control_replies_host(c.b.dec, c.b.seg_off[0], desc, res[0], mf)
    assert (n, got, tuple(rec), state) == (2, b"\x8a\x00", (1, 0, 0, 2), 0)
