"""The deflate rule (util_amd/csrc/ws_deflate.h: one fixed-Huffman block of LZ77 tokens per message,
the verdict, what is written to the room) compiled for the host and judged by deflate_oracle.py —
CPython's zlib inflates every DEFLATED body, websocketframeInflateHost does the same, the verdict
follows from the encoded length the rule reports — on the directed table (deflate_cases.py), at the
edges of min_len and of the room, on lists and on a seeded sweep; the exported host entry points;
the stand-alone sanitizer build; the symbol table of libwsframe_amd_pmd.so. CPU only: g++, ctypes
and numpy."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deflate_cases as DC
import deflate_oracle as O
import inflate_cases as IC
import send_cases as SC
import send_oracle as S
from test_abi import dynamic_symbols
from util_amd import _lib
from util_amd import wsframe as W

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "deflate_host.cpp")
GAP = 24                              # sentinel bytes on both sides of every room


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("deflate") / "libdeflate_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so_path], check=True)
    lib = C.CDLL(so_path)
    vp, u32, u64 = C.c_void_p, C.c_uint, C.c_ulonglong
    lib.ws_deflate_host_list.restype = C.c_longlong
    lib.ws_deflate_host_list.argtypes = [vp, u64, vp, u32, u64, vp, vp, vp, vp, vp]
    lib.ws_deflate_host_send_entry.restype = None
    lib.ws_deflate_host_send_entry.argtypes = [u32, vp, vp]
    lib.ws_deflate_host_sizes.restype = None
    lib.ws_deflate_host_sizes.argtypes = [vp]
    return lib


@pytest.fixture(scope="module")
def table():
    return DC.directed_table()


def entry_fn():
    lib = _lib.load_pmd_lib()

    def call(s, n, msg, nmsg, min_len, dst, off, cap, mr, enc):
        return lib.websocketframeDeflateHost(s, n, msg, nmsg, min_len, 0, dst, off, cap, mr)
    return call


def run_list(fn, src, lst, caps, min_len=0, room_shift=0):
    """a list [(src_off, len, type)] with one room per entry (caps), a sentinel gap around every
    room, the first room room_shift bytes into a 16-B aligned buffer: (return value, MSGRES records,
    enc_len per entry, destination, room offsets)"""
    src = np.ascontiguousarray(src, np.uint8)
    n = len(lst)
    msg = np.zeros(max(1, n), O.MSG_DTYPE)
    for i, e in enumerate(lst):
        msg[i] = e + (0,)
    offs, at = [], 32 + room_shift
    for c in caps:
        offs.append(at)
        at += c + GAP + 3
    raw = np.full(at + GAP + 16, O.FILL, np.uint8)
    a = (-raw.ctypes.data) % 16
    dst = raw[a:]
    off, cap = np.array(offs + [0], np.uint64), np.array(list(caps) + [0], np.uint64)
    mr = np.frombuffer(bytes([0xEE]) * (24 * max(1, n)), O.MSGRES_DTYPE).copy()
    enc = np.zeros(max(1, n), np.uint64)
    pad = np.zeros(1, np.uint8)
    r = fn((src if len(src) else pad).ctypes.data, len(src), msg.ctypes.data, n, min_len, dst.ctypes.data, off.ctypes.data,
           cap.ctypes.data, mr.ctypes.data, enc.ctypes.data)
    return r, mr[:n], enc[:n], dst, offs


def check_list(fn, src, lst, caps, min_len=0, room_shift=0, tag="", with_enc=True):
    """every entry of the list judged; nothing outside the rooms written. Returns the records."""
    r, mr, enc, dst, offs = run_list(fn, src, lst, caps, min_len, room_shift)
    keep = np.ones(len(dst), bool)
    sent = 0
    for i, ((o, n, t), cap) in enumerate(zip(lst, caps)):
        keep[offs[i]:offs[i] + cap] = False
        st, ol = int(mr[i]["status"]), int(mr[i]["out_len"])
        assert int(mr[i]["out_off"]) == offs[i] and int(mr[i]["reserved"]) == 0, tag
        if t == O.SKIP:
            assert (st, ol) == (O.SKIPPED, 0) and (dst[offs[i]:offs[i] + cap] == O.FILL).all(), tag
        elif o + n > len(src):
            assert (st, ol) == (O.ERR_RANGE, 0) and (dst[offs[i]:offs[i] + cap] == O.FILL).all(), tag
        else:
            O.judge(bytes(src[o:o + n]), min_len, cap, st, ol, dst[offs[i]:offs[i] + cap], int(enc[i]) if with_enc else None,
                    "%s entry %d" % (tag, i))
            sent += st in (O.DEFLATED, O.PLAIN)
    assert (dst[keep] == O.FILL).all(), tag + ": bytes outside the rooms written"
    assert r == sent, tag
    return mr, enc


def one(fn, data, cap=None, min_len=0, tag="", **kw):
    cap = max(len(data), 1) if cap is None else cap
    mr, enc = check_list(fn, np.frombuffer(data, np.uint8), [(0, len(data), 1)], [cap], min_len, tag=tag, **kw)
    return int(mr[0]["status"]), int(mr[0]["out_len"]), int(enc[0])


# ------------------------------------------------------------------ the rule, judged

def test_directed_table(host, table):
    entry = entry_fn()
    seen = set()
    for name, body in table:
        a = one(host.ws_deflate_host_list, body, tag="header, " + name)
        b = one(entry, body, tag="entry point, " + name, with_enc=False)
        assert a[:2] == b[:2], name
        seen.add(a[0])
        if len(body) == 0:
            assert a == (O.PLAIN, 0, 0)
    assert seen == {O.DEFLATED, O.PLAIN}
    results = {name: one(host.ws_deflate_host_list, body) for name, body in table}
    assert results["random 5000"][0] == O.PLAIN and results["random 5000"][2] > 5000
    for n in (257, 258, 259, 260, 516):
        assert results["one value, %d" % n][0] == O.DEFLATED


def test_inflate_host_reads_what_deflate_host_writes(table):
    """the library's own receive side gives the message back"""
    for name, body in table:
        if not 0 < len(body) <= 20000:
            continue
        dst, mr, n = W.deflate_host(np.frombuffer(body, np.uint8), np.array([(0, len(body), 2, 0)], W.DEFLATE_MSG_DTYPE), [5],
                                    [len(body)], len(body) + 5)
        assert n == 1
        if int(mr[0]["status"]) == W.DEFLATE_DEFLATED:
            out, imr, res = W.inflate_host(dst[5:5 + int(mr[0]["out_len"])],
                                           np.array([(0, int(mr[0]["out_len"]), W.INFLATE_RAW, 0)], W.INFLATE_MSG_DTYPE), len(body))
            assert int(res["status"]) == W.INFLATE_OK and out == body, name


def body_of(fn, data):
    r, mr, enc, dst, offs = run_list(fn, np.frombuffer(data, np.uint8), [(0, len(data), 1)], [len(data)])
    assert int(mr[0]["status"]) == O.DEFLATED
    return bytes(dst[offs[0]:offs[0] + int(mr[0]["out_len"])])


def test_tokens_walked(host, table):
    """the block's shape and every match's limits, by a fixed-Huffman reader of the test's own"""
    t = dict(table)
    fn = host.ws_deflate_host_list
    for name in ("one value, 257", "one value, 258", "one value, 259", "one value, 260", "one value, 516", "text of 4096",
                 "bytes 144-255", "period 3, 1000", "period 65, 700", "one value, 127", "one value, 129"):
        toks = O.tokens(body_of(fn, t[name]))
        assert O.replay(toks) == t[name], name
    # the maximum match and its split: 516 bytes of one value hold a match of 258
    assert any(isinstance(x, tuple) and x[0] == 258 for x in O.tokens(body_of(fn, t["one value, 516"])))
    # 9-bit literals: 112 of them before the first match can be found
    toks = O.tokens(body_of(fn, t["bytes 144-255"]))
    assert toks[:112] == list(range(144, 256)) and any(isinstance(x, tuple) for x in toks)
    # the far repeat: found at 32,768, not used at 32,769 (literals or a nearer match)
    for n in (3, 4):
        for dist in (32768, 32769):
            data = t["%d-byte repeat at distance %d" % (n, dist)]
            toks = O.tokens(body_of(fn, data))
            assert O.replay(toks) == data
            dists = [x[1] for x in toks if isinstance(x, tuple)]
            assert max(dists) <= 32768
            assert ((4, 32768) in [x for x in toks if isinstance(x, tuple)]) == (n == 4 and dist == 32768), (n, dist)


@pytest.mark.parametrize("n", [4096, 16384])
def test_honesty_floor_on_text(host, n):
    """at least half of what zlib saves with the same code (level 1, Z_FIXED) on the same text"""
    data = IC.text(np.random.default_rng(1), n)
    zf = len(IC.deflate(data, 1, zlib.Z_FIXED))
    st, out_len, enc = one(host.ws_deflate_host_list, data)
    print("text of %d: %d bytes, zlib level 1 Z_FIXED %d, level 1 %d" % (n, out_len, zf, len(IC.deflate(data, 1))))
    assert st == O.DEFLATED and out_len <= (n + zf) / 2


def test_min_len_edges(host):
    entry = entry_fn()
    data = IC.text(np.random.default_rng(2), 300)
    for fn, we in ((host.ws_deflate_host_list, True), (entry, False)):
        assert one(fn, data, min_len=299, with_enc=we)[0] == O.DEFLATED
        assert one(fn, data, min_len=300, with_enc=we)[0] == O.DEFLATED
        assert one(fn, data, min_len=301, with_enc=we)[:2] == (O.PLAIN, 300)
        assert one(fn, b"", min_len=0, cap=0, with_enc=we)[:2] == (O.PLAIN, 0)
        assert one(fn, data, min_len=301, cap=299, with_enc=we)[:2] == (O.ERR_OUT_SPACE, 0)


def test_room_edges(host):
    """cap at out_len - 1 and out_len, for a DEFLATED and a PLAIN message"""
    entry = entry_fn()
    good, bad = IC.text(np.random.default_rng(2), 700), DC.rnd(3, 700)
    for fn, we in ((host.ws_deflate_host_list, True), (entry, False)):
        st, n, enc = one(fn, good, with_enc=we)
        assert st == O.DEFLATED and n < 700
        assert one(fn, good, cap=n, with_enc=we)[:2] == (O.DEFLATED, n)
        assert one(fn, good, cap=n - 1, with_enc=we)[:2] == (O.ERR_OUT_SPACE, 0)
        assert one(fn, good, cap=0, with_enc=we)[:2] == (O.ERR_OUT_SPACE, 0)
        assert one(fn, bad, cap=700, with_enc=we)[:2] == (O.PLAIN, 700)
        assert one(fn, bad, cap=699, with_enc=we)[:2] == (O.ERR_OUT_SPACE, 0)
        assert one(fn, good, cap=5000, with_enc=we)[:2] == (O.DEFLATED, n)


def test_lists_skips_and_ranges(host):
    entry = entry_fn()
    rng = np.random.default_rng(6)
    src = np.frombuffer(IC.text(rng, 900) + DC.rnd(7, 300) + b"z" * 400, np.uint8)
    n = len(src)
    skip = (n + 5, 1 << 40, O.SKIP)
    lst = [(0, 900, 1), skip, (900, 300, 2), (0, 0, O.SKIP), (1200, 400, 1), (n - 3, 4, 2), (n - 4, 4, 2), (1 << 63, 1 << 63, 1),
           (0, n, 2), (n, 0, 1), (n + 1, 0, 1)]
    caps = [900, 50, 300, 0, 400, 10, 10, 10, n, 0, 4]
    for fn, we in ((host.ws_deflate_host_list, True), (entry, False)):
        mr, _ = check_list(fn, src, lst, caps, tag="list", with_enc=we)
        assert [int(v) for v in mr["status"]] == [O.DEFLATED, O.SKIPPED, O.PLAIN, O.SKIPPED, O.DEFLATED, O.ERR_RANGE, O.PLAIN,
                                                  O.ERR_RANGE, O.DEFLATED, O.PLAIN, O.ERR_RANGE]
        check_list(fn, src, [], [], tag="empty list", with_enc=we)


def test_every_source_and_room_offset(host):
    """source offsets 0 to 15 and room offsets 0 to 15: the same body comes out at each"""
    data = IC.text(np.random.default_rng(8), 333)
    src = np.frombuffer(bytes(16) + data + bytes(16), np.uint8)
    want = None
    for so in range(16):
        buf = np.frombuffer(bytes([7]) * so + data + bytes([9]) * 16, np.uint8)
        for ro in range(16):
            r, mr, enc, dst, offs = run_list(host.ws_deflate_host_list, buf, [(so, 333, 1)], [333], room_shift=ro)
            n = int(mr[0]["out_len"])
            got = bytes(dst[offs[0]:offs[0] + n])
            want = want or got
            assert int(mr[0]["status"]) == O.DEFLATED and got == want and offs[0] % 16 == ro
            assert (dst[:offs[0]] == O.FILL).all() and (dst[offs[0] + 333:] == O.FILL).all()
    assert O.inflate(want) == data and len(src)


def test_send_map(host):
    fn = host.ws_deflate_host_send_entry
    for typ in (1, 2, 0x1F2, O.SKIP):
        for st in range(5):
            r = np.zeros(1, O.MSGRES_DTYPE)
            r[0] = (1000, 77, st, 0)
            out = np.zeros(1, O.MSG_DTYPE)
            fn(typ, r.ctypes.data, out.ctypes.data)
            assert (int(out[0]["src_off"]), int(out[0]["len"]), int(out[0]["type"])) == O.send_entry(typ, st, 1000, 77)
            assert int(out[0]["reserved"]) == 0
    assert O.send_entry(1, O.DEFLATED, 5, 6) == (5, 6, 0x41) and O.send_entry(1, O.PLAIN, 5, 6) == (5, 6, 1)
    assert O.send_entry(1, O.ERR_RANGE, 5, 6) == (0, 0, O.SKIP)


def test_send_ext_host():
    """flag 1: RSV1 on the first frame only, over one to many frames, in both roles; flag 0 and
    every unmarked entry: websocketframeSendHost's bytes"""
    src = SC.source()
    conn = [(0, 0, 0x41), (10, 5, 0x42), (100, 300, 0x41), (50, 1000, 1), (7, 0, O.SKIP), (2000, 700, 0x1F2), (9, 9, 0x4A)]
    for role in (False, True):
        keys = SC.keys_for(dict(role=role, conns=[conn]), len(conn))
        for F in (S.FRAG_DEFAULT, 130 + 4 * role, 7 + 4 * role):
            etx, eoff, emoff, eres = O.send_ext(src, [conn], [F], keys, len(conn))
            plain = S.batch(src, [conn], [F], keys, len(conn))[0]
            msg = np.array([e + (0,) for e in conn], W.SEND_MSG_DTYPE)
            tx, moff, res = W.send_ext_host(src, msg, F, keys, flags=1)
            assert tx == bytes(etx) and res == eres[0]
            diff = np.flatnonzero(np.frombuffer(tx, np.uint8) != np.asarray(plain, np.uint8))
            assert [int(d) for d in diff] == [int(emoff[i]) for i, e in enumerate(conn) if e[2] != O.SKIP and e[2] & 0x40]
            if F == 7 + 4 * role:
                assert int(res["n_frames"]) > 3 * len(conn)          # the marked messages span many frames
            tx0, _, res0 = W.send_ext_host(src, msg, F, keys, flags=0)
            n, old, _, res_old = W.send_host(src, msg, F, keys)
            assert tx0 == old == bytes(np.asarray(plain, np.uint8)) and res0 == res_old
    lib = _lib.load_pmd_lib()
    out = np.zeros(1, W.SEND_RES_DTYPE)
    assert lib.websocketframeSendExtHost(src.ctypes.data, len(src), None, 0, 100, None, 2, None, 0, None, out.ctypes.data) < 0
    assert b"flag" in lib.websocketframeGpuLastError()
    assert lib.websocketframeSendHost(src.ctypes.data, len(src), None, 0, 100, None, 1, None, 0, None, out.ctypes.data) < 0


def test_sweep_through_the_library(host):
    """a few hundred sweep bodies through the shared object, judged by zlib (the sanitizer program
    below runs thousands and inflates them itself)"""
    bodies = DC.sweep(400, seed=21, max_len=20000)
    seen = {O.DEFLATED: 0, O.PLAIN: 0}
    for k, b in enumerate(bodies):
        seen[one(host.ws_deflate_host_list, b, tag="sweep %d" % k)[0]] += 1
    print("sweep:", seen)
    assert seen[O.DEFLATED] >= 100 and seen[O.PLAIN] >= 50


# ------------------------------------------------------------------ the stand-alone program

def test_host_program_under_sanitizers(tmp_path, table):
    """the same source as a program of its own, built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as its own process: source and room are exactly as long as
    they are said to be, every DEFLATED body is inflated again by ws_inflate.h"""
    exe = str(tmp_path / "deflate_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DDEFLATE_HOST_MAIN", SRC, "-o", exe], check=True)
    bodies = [b for _, b in table] + DC.sweep(3000)
    rng = np.random.default_rng(5)
    blobs = []
    for k, body in enumerate(bodies):
        n = len(body)
        cap = [n, max(n, 1), n + 7, max(0, n - 1), n // 2, 0][k % 6] if k % 4 == 0 else max(n, 1)
        min_len = [0, n, n + 1, max(0, n - 1), 64][k % 5] if k % 3 == 0 else 0
        blobs.append(struct.pack("<3I", n, min_len, cap) + body)
    assert len(blobs) >= 3000 and max(len(b) for b in bodies) >= 65000 and rng is not None
    with open(str(tmp_path / "cases.bin"), "wb") as f:
        f.write(struct.pack("<I", len(blobs)) + b"".join(blobs))
    out = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("deflate_host ok: %d cases" % len(blobs)), out.stdout + out.stderr
    counts = [int(v) for v in re.findall(r"(\d+) (?:deflated|plain|out of space)", out.stdout)]
    assert min(counts) >= 100, out.stdout


# ------------------------------------------------------------------ ABI, arguments

def test_pmd_library_exports():
    """libwsframe_amd_pmd.so's symbol table is libwsframe_amd_deflate.so's plus exactly the names
    wsframe_amd_compress.h marks; the older libraries export none of them"""
    text = open(os.path.join(_lib.REPO, "include", "wsframe_amd_compress.h")).read()
    marked = set(re.findall(r"WSFRAME_AMD_PMD_EXPORT[^;]*?\b(websocketframe\w+)\s*\(", text, re.S))
    assert marked == set(_lib.PMD_EXPORTS) and len(marked) == 5
    assert os.path.exists(_lib.PMD_LIB_PATH), "libwsframe_amd_pmd.so is not built"
    assert dynamic_symbols(_lib.PMD_LIB_PATH) == dynamic_symbols(_lib.DEFLATE_LIB_PATH) | marked
    for path in (_lib.LIB_PATH, _lib.CTL_LIB_PATH, _lib.TEXT_LIB_PATH, _lib.PROTO_LIB_PATH, _lib.HS_LIB_PATH, _lib.REPLY_LIB_PATH,
                 _lib.SEND_LIB_PATH, _lib.CLI_LIB_PATH, _lib.DEFLATE_LIB_PATH, _lib.BENCH_LIB_PATH):
        assert not dynamic_symbols(path) & marked, path


def test_constants_and_struct_layout(host, tmp_path):
    text = open(os.path.join(_lib.REPO, "include", "wsframe_amd_compress.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"WEBSOCKET_DEFLATE_(\w+) = (\d+)", text)}
    assert enum == {"DEFLATED": 0, "PLAIN": 1, "SKIPPED": 2, "ERR_OUT_SPACE": 3, "ERR_RANGE": 4}
    for name, value in enum.items():
        assert getattr(W, "DEFLATE_" + name) == value == getattr(O, name)
    defs = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define WEBSOCKET_SEND_(FLAG_RSV1|TYPE_RSV1)\s+(\w+)", text)}
    assert defs == {"FLAG_RSV1": 1, "TYPE_RSV1": 0x40} and (W.SEND_FLAG_RSV1, W.SEND_TYPE_RSV1) == (O.RSV1_FLAG, O.RSV1_TYPE) == (1, 0x40)
    assert (W.DEFLATE_MSG_DTYPE, W.DEFLATE_MSGRES_DTYPE) == (O.MSG_DTYPE, O.MSGRES_DTYPE) and W.DEFLATE_MSG_DTYPE == W.SEND_MSG_DTYPE
    v = np.zeros(8, np.uint32)
    host.ws_deflate_host_sizes(v.ctypes.data)
    assert [int(x) for x in v] == [24, 8, 24, 8, 8456, 64, 4, 11]
    prog = tmp_path / "size.c"
    prog.write_text('#include "wsframe_amd_compress.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { '
                    'printf("%zu %zu %zu %zu %zu %zu %zu %u %u %d", sizeof(WebsocketDeflateMsg_t), sizeof(WebsocketSendMsg_t), '
                    "offsetof(WebsocketDeflateMsg_t, type), sizeof(WebsocketDeflateMsgRes_t), _Alignof(WebsocketDeflateMsgRes_t), "
                    "offsetof(WebsocketDeflateMsgRes_t, out_len), offsetof(WebsocketDeflateMsgRes_t, status), "
                    "WEBSOCKET_SEND_FLAG_RSV1, WEBSOCKET_SEND_TYPE_RSV1, WEBSOCKET_DEFLATE_ERR_RANGE); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(_lib.REPO, "include"), str(prog), "-o", exe],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "24 24 16 24 8 8 16 1 64 4"


def test_entry_point_refuses_bad_arguments():
    lib = _lib.load_pmd_lib()
    body = np.frombuffer(b"hello " * 30, np.uint8)                 # (three groups: the second finds the first)
    msg = np.zeros(1, O.MSG_DTYPE)
    msg[0] = (0, len(body), 1, 0)
    dst = np.full(256, O.FILL, np.uint8)
    off, cap = np.zeros(1, np.uint64), np.full(1, 256, np.uint64)
    mr = np.full(6, 7, np.uint32)

    def call(s=body.ctypes.data, n=len(body), m=msg.ctypes.data, flags=0, o=off.ctypes.data, c=cap.ctypes.data, r=mr.ctypes.data):
        return lib.websocketframeDeflateHost(s, n, m, 1, 0, flags, dst.ctypes.data, o, c, r)
    for kw, word in ((dict(flags=1), b"flag"), (dict(s=None), b"NULL"), (dict(m=None), b"NULL"), (dict(o=None), b"NULL"),
                     (dict(c=None), b"NULL"), (dict(r=None), b"NULL")):
        assert call(**kw) < 0 and word in lib.websocketframeGpuLastError(), kw
        assert (dst == O.FILL).all() and (mr == 7).all()
    assert call() == 1
    r = mr.view(O.MSGRES_DTYPE)[0]
    assert int(r["status"]) == O.DEFLATED and O.inflate(dst[:int(r["out_len"])]) == body.tobytes()
    assert (dst[int(r["out_len"]):] == O.FILL).all()
