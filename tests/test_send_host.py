"""The batch message send's rule (util_amd/csrc/ws_send.h: the shard, the closed-form lengths, the
byte function, the slot summary and its combine, the workspace layout) compiled for the host and
held against the sequential model (send_oracle.py: the reference's sharding loop line by line, the
oracle's encoder for the header bytes) on the directed table and random lists (send_cases.py); the
exported host entry point against the same; the wire bytes through the oracle's decoder and through
the reference's own rx stack; the stand-alone sanitizer build; the symbol table of
libwsframe_amd_send.so. CPU only: g++, ctypes and numpy."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ref_reactor
import send_cases as SC
import send_oracle as S
from oracle_lib import oracle_segments
from test_abi import dynamic_symbols
from util_amd import _lib
from util_amd import wsframe as W

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "send_host.cpp")
PAD = 32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("send") / "libsend_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so_path], check=True)
    lib = C.CDLL(so_path)
    vp, u32, u64 = C.c_void_p, C.c_uint, C.c_ulonglong
    lib.ws_send_host_connection.restype = C.c_longlong
    lib.ws_send_host_connection.argtypes = [vp, u64, vp, u32, u32, vp, vp, u64, vp, vp]
    lib.ws_send_host_runs.restype = C.c_longlong
    lib.ws_send_host_runs.argtypes = [vp, u64, vp, u32, u32, vp, vp, u64, vp, vp, vp, u32]
    lib.ws_send_host_assoc.restype = u32
    lib.ws_send_host_assoc.argtypes = [vp, u32, u32, u32, u64, u32, u32]
    lib.ws_send_host_geo.restype = u32
    lib.ws_send_host_geo.argtypes = [u64, u32, u32, vp]
    lib.ws_send_host_frag_key.restype = u32
    lib.ws_send_host_frag_key.argtypes = [u32, u64]
    lib.ws_send_host_layout.restype = None
    lib.ws_send_host_layout.argtypes = [u32, u32, u64, vp]
    lib.ws_send_host_pieces.restype = u64
    lib.ws_send_host_pieces.argtypes = [u64, u32]
    lib.ws_send_host_sizes.restype = u32
    return lib


@pytest.fixture(scope="module")
def src():
    return SC.source()


@pytest.fixture(scope="module")
def table(src):
    """every directed case with the model's answer, computed once"""
    return [(c,) + SC.expect(c, src) for c in SC.directed_table()]


@pytest.fixture(scope="module")
def randoms(src):
    return [(c,) + SC.expect(c, src) for c in SC.random_cases()]


def entry_fn():
    lib = _lib.load_send_lib()

    def call(s, n, msg, nmsg, F, keys, tx, cap, moff, out):
        return lib.websocketframeSendHost(s, n, msg, nmsg, F, keys, 0, tx, cap, moff, out)
    return call


def run_connection(fn, src, msg, n, F, keys, cap=None, cuts=None, total=0):
    """connection through one of the C routines. Returns (length, tx bytes that fit, msg offsets,
    result tuple, the bytes past them: all FILL)"""
    msg = np.ascontiguousarray(msg[:n])
    k = None if keys is None else np.ascontiguousarray(keys[:n])
    cap = total if cap is None else cap
    tx = np.full(cap + 16, S.FILL, np.uint8)
    moff = np.full(max(1, n), 0xEEEEEEEEEEEEEEEE, np.uint64)
    out = np.zeros(1, S.RES_DTYPE)
    args = [src.ctypes.data, len(src), msg.ctypes.data if n else None, n, F, None if k is None else k.ctypes.data,
            tx.ctypes.data, cap, moff.ctypes.data, out.ctypes.data]
    if cuts is not None:
        ca = np.asarray(cuts, np.uint32)
        args += [ca.ctypes.data, len(ca)]
    got = fn(*args)
    fit = min(max(got, 0), cap)
    return got, tx[:fit], moff[:n], tuple(int(v) for v in out[0]), tx[fit:]


def check_connection(got, exp, s, mm, n, tag):
    length, tx, moff, res, rest = got
    etx, eoff, emoff, eres = exp
    lo, hi = int(eoff[s]), int(eoff[s + 1])
    assert length == hi - lo, "%s connection %d: length %d, expected %d" % (tag, s, length, hi - lo)
    assert np.array_equal(tx, etx[lo:lo + len(tx)]), "%s connection %d: wire bytes differ" % (tag, s)
    assert res == tuple(int(v) for v in eres[s]), "%s connection %d: result %s, expected %s" % (tag, s, res, eres[s])
    assert np.array_equal(moff, emoff[s * mm:s * mm + n] - np.uint64(lo)), "%s connection %d: message offsets" % (tag, s)
    assert (rest == S.FILL).all(), "%s connection %d: bytes past the wire written" % (tag, s)


def all_connections(cases):
    for c, msg, nmsg, mm, keys, exp in cases:
        for s in range(len(c["conns"])):
            yield c, s, msg[s * mm:(s + 1) * mm], int(nmsg[s]), mm, int(c["frags"][s]), None if keys is None else keys[s * mm:(s + 1) * mm], exp


# ------------------------------------------------------------------ 1: header and entry point vs the model

def test_table_covers_what_it_says(table):
    """the table against the issue's list (fragment sizes of both roles, every status, every opcode);
    the shard values are literals worked out by hand from the reference's loop"""
    fs = {(c["role"], f) for c, *_ in table for f in c["frags"]}
    for f in SC.SERVER_F:
        assert (False, f) in fs
    for f in SC.CLIENT_F:
        assert (True, f) in fs
    st = {int(v) for *_, exp in table for v in exp[3]["status"]}
    assert st == {S.OK, S.ERR_FRAGMENT_SIZE, S.ERR_RANGE}
    types = {t & 15 for c, *_ in table for conn in c["conns"] for (_, _, t) in conn if t != S.SKIP}
    assert types == set(range(16))
    # the quirk: the header length is taken at F
    assert [S.shard_of(f, False) for f in (125, 126, 65536)] == [123, 122, 65526]
    assert [S.shard_of(f, True) for f in (6, 7, 125, 129, 130)] == [0, 1, 119, 121, 122]


def test_header_and_entry_point_give_the_table(host, src, table):
    entry = entry_fn()
    for c, s, msg, n, mm, F, keys, exp in all_connections(table):
        total = int(exp[1][s + 1] - exp[1][s])
        for fn, name in ((host.ws_send_host_connection, "header"), (entry, "entry point")):
            check_connection(run_connection(fn, src, msg, n, F, keys, total=total), exp, s, mm, n, "%s, %s" % (name, c["name"]))
        check_connection(run_connection(host.ws_send_host_runs, src, msg, n, F, keys, cuts=[n // 2], total=total), exp, s, mm, n,
                         "runs, %s" % c["name"])


def test_header_and_entry_point_match_the_model_on_random_lists(host, src, randoms):
    entry = entry_fn()
    rng = np.random.default_rng(3)
    seen = set()
    for c, s, msg, n, mm, F, keys, exp in all_connections(randoms):
        total = int(exp[1][s + 1] - exp[1][s])
        seen.add(int(exp[3][s]["status"]))
        check_connection(run_connection(host.ws_send_host_connection, src, msg, n, F, keys, total=total), exp, s, mm, n, c["name"])
        check_connection(run_connection(entry, src, msg, n, F, keys, total=total), exp, s, mm, n, "entry point, " + c["name"])
        cuts = sorted(int(v) for v in rng.integers(0, n + 2, int(rng.integers(0, 4))))
        check_connection(run_connection(host.ws_send_host_runs, src, msg, n, F, keys, cuts=cuts, total=total), exp, s, mm, n,
                         "runs %s, %s" % (cuts, c["name"]))
    assert seen == {S.OK, S.ERR_FRAGMENT_SIZE, S.ERR_RANGE}


def test_capacity_cuts(host, src, table):
    """capacities around the header bytes, the middle and the end: the length and the result do
    not change, no byte at or past the capacity is written"""
    entry = entry_fn()
    for c, s, msg, n, mm, F, keys, exp in all_connections(table):
        total = int(exp[1][s + 1] - exp[1][s])
        if not 0 < total <= 5000:
            continue
        for cap in sorted({0, 1, 2, 3, 5, 6, 7, 13, total // 2, total - 1, total, total + 1}):
            for fn in (host.ws_send_host_connection, entry):
                check_connection(run_connection(fn, src, msg, n, F, keys, cap=cap), exp, s, mm, n, "cap %d, %s" % (cap, c["name"]))


def test_closed_form_lengths(host):
    """shard, frames and wire bytes against the formulas written out in the model and, where the
    loop is short enough, against the loop itself; lengths past 2^32 included"""
    rng = np.random.default_rng(5)
    Fs = sorted(set(SC.SERVER_F + SC.CLIENT_F + [int(v) for v in rng.integers(0, 1 << 17, 40)] + [1 << 31, (1 << 32) - 2]))
    Ls = [0, 1, 2, 121, 122, 123, 124, 125, 126, 127, 65535, 65536, 65537, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 12345]
    for role in (0, 1):
        for F in Fs:
            shard = S.shard_of(F, role)
            for L in Ls + ([shard - 1, shard, shard + 1, 2 * shard, 5 * shard + 1] if shard else []):
                out = np.zeros(3, np.uint64)
                ok = host.ws_send_host_geo(L, F, role, out.ctypes.data)
                want = S.closed_form(L, F, role)
                assert int(out[0]) == shard and bool(ok) == (want is not None), (L, F, role)
                if want is None:
                    continue
                assert (int(out[1]), int(out[2])) == want, (L, F, role)
                if want[0] <= 2000:
                    pk = S.shard_packets(L, F, role)
                    assert (len(pk), sum(h + b for h, b, _ in pk)) == want, (L, F, role)
    for key, j in ((0, 0), (0x01020304, 0), (0x01020304, 1), (0xFFFFFFFF, 7), (5, (1 << 32) + 3)):
        assert host.ws_send_host_frag_key(key, j) == S.frag_key(key, j & 0xFFFFFFFF)
    assert S.frag_key(0x01020304, 1) == 0x01020304 ^ 0x9E3779B9


def test_combine_is_associative_on_random_runs(host):
    rng = np.random.default_rng(65)
    for _ in range(5000):
        na, nb, nc = (int(v) for v in rng.integers(0, 5, 3))
        n = max(1, na + nb + nc)
        msg = np.zeros(n, S.MSG_DTYPE)
        msg["src_off"] = rng.integers(0, 1200, n)
        msg["len"] = rng.choice([0, 1, 10, 200, 900], n)
        msg["type"] = rng.choice([1, 2, S.SKIP], n)
        F = int(rng.choice([2, 3, 50, 0xFFFFFFFF]))
        assert host.ws_send_host_assoc(msg.ctypes.data, na, nb, nc, 1000, F, int(rng.integers(0, 2))) == 0, (msg, na, nb, nc, F)


# ------------------------------------------------------------------ 2: through the decoders

def decode_stream(tx):
    """wire bytes as one segment through the oracle's decoder: [(type, is_fin, plain body)]"""
    buf = np.concatenate([np.asarray(tx, np.uint8), np.zeros(PAD, np.uint8)])
    desc, res = oracle_segments(buf, [0], [len(tx)], 1 << 17)
    assert int(res[0]["consumed"]) == len(tx) and int(res[0]["status"]) == 0
    out = []
    for d in desc[:int(res[0]["n_frames"])]:
        n = int(d["datalen"])
        out.append((int(d["type"]), int(d["is_fin"]), buf[int(d["data_off"]):int(d["data_off"]) + n] if n else buf[:0]))
    return out


def messages_of(frames):
    """frames folded into messages: [(opcode, body bytes)]; a continuation joins the open message"""
    msgs, cur = [], None
    for typ, fin, body in frames:
        if cur is None:
            cur = [typ, [body]]
        else:
            assert typ == 0, "a fragment after the first is a continuation"
            cur[1].append(body)
        if fin:
            msgs.append((cur[0], np.concatenate(cur[1]).tobytes()))
            cur = None
    assert cur is None, "the last message is closed"
    return msgs


def built(fn, src, msg, n, F, keys, total):
    """the wire bytes the C code itself builds for a connection (not the model's)"""
    length, tx, _moff, _res, _rest = run_connection(fn, src, msg, n, F, keys, total=total)
    assert length == total == len(tx)
    return tx


@pytest.mark.parametrize("which", ["table", "random"])
def test_wire_bytes_decode_to_the_messages(host, src, table, randoms, which):
    """every connection's bytes as the exported host entry point builds them, server role and
    masked, through the oracle's decoder (which unmasks): exactly the input messages, in order,
    each fragment no larger than the shard"""
    nmsgs = 0
    entry = entry_fn()
    for c, s, msg, n, mm, F, keys, exp in all_connections(table if which == "table" else randoms):
        lo, hi = int(exp[1][s]), int(exp[1][s + 1])
        if hi - lo > 300000 or (S.shard_of(F, c["role"]) or 1) < 3 and hi - lo > 30000:
            continue
        frames = decode_stream(built(entry, src, msg, n, F, keys, hi - lo))
        assert len(frames) == int(exp[3][s]["n_frames"])
        shard = S.shard_of(F, c["role"])
        assert all(len(b) <= shard for _, _, b in frames if len(b))
        want = [] if int(exp[3][s]["status"]) else [(t & 15, src[o:o + ln].tobytes()) for (o, ln, t) in c["conns"][s] if t != S.SKIP]
        assert messages_of(frames) == want, (c["name"], s)
        nmsgs += len(want)
    assert nmsgs >= 100


@pytest.mark.parametrize("chunk", [7, 1500])
def test_reference_rx_stack_delivers_the_messages(host, src, table, randoms, chunk):
    """server-role bytes, as ws_send.h's routine and the exported host entry point build them (in
    turn), through the reference's rx stack (the reactor,
    its stream hook and fragment cache, the reference's decoder), fed in `chunk`-byte writes: it
    delivers exactly the input messages, in order, with nothing pending"""
    assert ref_reactor.available(), "the reference reactor is not built: __graft_entry__.build() makes it"
    done = 0
    for c, s, msg, n, mm, F, keys, exp in all_connections(table + randoms):
        lo, hi = int(exp[1][s]), int(exp[1][s + 1])
        if c["role"] or hi == lo or hi - lo > (20000 if chunk == 7 else 400000):
            continue
        sent = [(o, ln) for (o, ln, t) in c["conns"][s] if t != S.SKIP]
        fn = host.ws_send_host_connection if done % 2 else entry_fn()
        r = ref_reactor.reactor_deliver(built(fn, src, msg, n, F, keys, hi - lo), chunk=chunk)
        assert r["detach_error"] == 0 and r["pending"] == 0 and r["cached"] == 0, (c["name"], s, r)
        assert r["consumed"] == hi - lo and r["frames"] == int(exp[3][s]["n_frames"])
        assert r["lens"] == [ln for _, ln in sent], (c["name"], s)
        body = np.concatenate([src[o:o + ln] for o, ln in sent]) if sent else np.zeros(0, np.uint8)
        assert np.array_equal(r["bodies"], body), (c["name"], s)
        done += 1
    assert done >= 20


# ------------------------------------------------------------------ 3: the stand-alone program

def case_file(path, src, cases):
    blobs = []
    for c, s, msg, n, mm, F, keys, exp in all_connections(cases):
        lo, hi = int(exp[1][s]), int(exp[1][s + 1])
        if hi - lo > 3000:
            continue
        head = struct.pack("<6I", len(src), n, F, int(keys is not None), hi - lo, int(exp[3][s]["status"]))
        blobs.append(head + src.tobytes() + msg[:n].tobytes() + (keys[:n].tobytes() if keys is not None else b"") +
                     exp[0][lo:hi].tobytes())
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blobs)) + b"".join(blobs))
    return len(blobs)


def test_host_program_under_sanitizers(tmp_path, src, table):
    """the same source as a program of its own, built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as its own process: source, list and wire buffer are exactly
    as long as they are said to be"""
    exe = str(tmp_path / "send_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DSEND_HOST_MAIN", SRC, "-o", exe], check=True)
    ncase = case_file(str(tmp_path / "table.bin"), src, table)
    assert ncase >= 40
    out = subprocess.run([exe, str(tmp_path / "table.bin")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("send_host ok: %d cases" % ncase), out.stdout + out.stderr


# ------------------------------------------------------------------ layout, ABI, arguments

def up(x, a):
    return (x + a - 1) // a * a


@pytest.mark.parametrize("nseg,mm,cap", [(1, 1, 0), (3, 7, 1), (255, 2, 16384), (256, 1, 16385), (257, 300, 1 << 20),
                                          (1000, 301, (1 << 20) - 15), (65536, 16, 1 << 32), (1 << 20, 1, 1 << 33),
                                          (1, 1 << 20, 123), (1 << 15, 1 << 15, 1 << 44)])
def test_workspace_layout(host, nseg, mm, cap):
    """ws_send.h's layout against the formulas written out here: regions in order, 16-B aligned,
    none overlapping, the sizes the kernels index; the piece count covers every phase of d_tx"""
    assert host.ws_send_host_sizes() == 32 | 48 << 8 | 32 << 16 | 24 << 24
    got = np.zeros(10, np.uint64)
    host.ws_send_host_layout(nseg, mm, cap, got.ctypes.data)
    nb, nt = (nseg + 255) // 256, (nseg * mm + 255) // 256
    npieces = ((cap + 15) >> 14) + 1 if cap else 0
    bo64 = 16
    loc = bo64 + up(8 * (nb + 1), 16)
    tail = loc + 8 * 256 * nb
    agg = tail + 32 * nseg
    rec = agg + 32 * nt
    ptr = rec + 48 * nseg * mm
    assert [int(v) for v in got] == [bo64, loc, tail, agg, rec, ptr, ptr + up(4 * npieces, 16), nb, nt, npieces]
    assert all(int(v) % 16 == 0 for v in got[:7])
    for lead in range(16):
        for limit in {0, 1, cap // 2, max(cap, 1) - 1, cap}:
            want = 0 if limit == 0 else (limit + lead - 1) // 16384 + 1
            assert host.ws_send_host_pieces(limit, lead) == want <= max(npieces, want if limit > cap else 0)


def test_send_library_exports():
    """libwsframe_amd_send.so's symbol table is libwsframe_amd_reply.so's plus exactly the names
    wsframe_amd_send.h marks; the older libraries export none of them"""
    text = open(os.path.join(_lib.REPO, "include", "wsframe_amd_send.h")).read()
    marked = set(re.findall(r"WSFRAME_AMD_SEND_EXPORT[^;]*?\b(websocketframe\w+)\s*\(", text, re.S))
    assert marked == set(_lib.SEND_EXPORTS) and len(marked) == 3
    assert os.path.exists(_lib.SEND_LIB_PATH), "libwsframe_amd_send.so is not built"
    assert dynamic_symbols(_lib.SEND_LIB_PATH) == dynamic_symbols(_lib.REPLY_LIB_PATH) | marked
    for path in (_lib.LIB_PATH, _lib.CTL_LIB_PATH, _lib.TEXT_LIB_PATH, _lib.PROTO_LIB_PATH, _lib.HS_LIB_PATH,
                 _lib.REPLY_LIB_PATH, _lib.BENCH_LIB_PATH):
        assert not dynamic_symbols(path) & marked, path


def test_constants_agree(tmp_path):
    text = open(os.path.join(_lib.REPO, "include", "wsframe_amd_send.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"WEBSOCKET_SEND_(OK|ERR_\w+) = (\d+)", text)}
    assert enum == {"OK": 0, "ERR_FRAGMENT_SIZE": 1, "ERR_RANGE": 2}
    for name, value in enum.items():
        assert getattr(W, "SEND_" + name) == value == getattr(S, name)
    defs = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define WEBSOCKET_SEND_(\w+)\s+(0x\w+)", text)}
    assert defs == {"SKIP": 0xFFFFFFFF, "NONE": 0xFFFFFFFF, "FRAG_DEFAULT": 0xFFFFFFFF}
    assert W.SEND_SKIP == S.SKIP and W.SEND_NONE == S.NONE and W.SEND_FRAG_DEFAULT == S.FRAG_DEFAULT
    assert W.SEND_MSG_DTYPE == S.MSG_DTYPE and W.SEND_RES_DTYPE == S.RES_DTYPE
    prog = tmp_path / "size.c"
    prog.write_text('#include "wsframe_amd_send.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu", '
                    "sizeof(WebsocketSendMsg_t), sizeof(WebsocketSendResult_t)); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(_lib.REPO, "include"), str(prog), "-o", exe],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "24 32"


def test_entry_point_refuses_bad_arguments(src):
    lib = _lib.load_send_lib()
    msg = np.zeros(1, S.MSG_DTYPE)
    msg[0] = (0, 3, 2, 0)
    tx = np.full(64, S.FILL, np.uint8)
    out = np.full(8, 7, np.uint32)

    def call(s=src.ctypes.data, n=len(src), m=msg.ctypes.data, flags=0, t=tx.ctypes.data, cap=64, o=out.ctypes.data):
        return lib.websocketframeSendHost(s, n, m, 1, 0xFFFFFFFF, None, flags, t, cap, None, o)
    for kw, word in ((dict(flags=1), b"flag"), (dict(s=None), b"NULL"), (dict(m=None), b"NULL"), (dict(o=None), b"NULL"),
                     (dict(t=None), b"NULL"), (dict(n=(1 << 56) + 1), b"src_len")):
        assert call(**kw) < 0 and word in lib.websocketframeGpuLastError(), kw
        assert (tx == S.FILL).all() and (out == 7).all()
    assert call(t=None, cap=0) == 5
    n, got, moff, rec = W.send_host(src, msg)
    assert (n, got, int(moff[0]), int(rec["n_frames"]), int(rec["status"])) == (5, bytes([0x82, 3]) + src[:3].tobytes(), 0, 1, 0)
