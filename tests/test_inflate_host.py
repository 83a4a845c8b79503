"""The inflate rule (util_amd/csrc/ws_inflate.h: raw DEFLATE over body + 00 00 FF FF judged where
zlib judges, the limits, the walk over a connection's list) compiled for the host and held against
the sequential model (inflate_oracle.py: CPython's zlib) on the directed table, every truncation of
one stream, every single-bit flip of another and seeded random bodies (inflate_cases.py); the
exported host entry point on lists; the stand-alone sanitizer build; the symbol table of
libwsframe_amd_deflate.so. CPU only: g++, ctypes and numpy."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import inflate_cases as IC
import inflate_oracle as O
from test_abi import dynamic_symbols
from util_amd import _lib
from util_amd import wsframe as W

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "inflate_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("inflate") / "libinflate_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so_path], check=True)
    lib = C.CDLL(so_path)
    vp, u32, u64 = C.c_void_p, C.c_uint, C.c_ulonglong
    lib.ws_inflate_host_connection.restype = C.c_longlong
    lib.ws_inflate_host_connection.argtypes = [vp, u64, vp, u32, u64, vp, u64, vp, vp]
    lib.ws_inflate_host_sizes.restype = None
    lib.ws_inflate_host_sizes.argtypes = [vp]
    return lib


def entry_fn():
    lib = _lib.load_deflate_lib()

    def call(s, n, msg, nmsg, limit, dst, cap, mr, out):
        return lib.websocketframeInflateHost(s, n, msg, nmsg, limit, 0, dst, cap, mr, out)
    return call


def run_list(fn, src, lst, limit=0, cap=0):
    """a connection's list [(src_off, len, kind)] through one of the C routines: (return value,
    output bytes, MSGRES records, RES record, the bytes behind the room: all FILL)"""
    src = np.ascontiguousarray(src, np.uint8)
    pad = np.zeros(1, np.uint8)
    msg = np.zeros(max(1, len(lst)), O.MSG_DTYPE)
    for i, e in enumerate(lst):
        msg[i] = e + (0,)
    dst = np.full(cap + 16, O.FILL, np.uint8)
    mr = np.frombuffer(bytes([0xEE]) * (24 * max(1, len(lst))), O.MSGRES_DTYPE).copy()
    out = np.zeros(1, O.RES_DTYPE)
    n = fn((src if len(src) else pad).ctypes.data, len(src), msg.ctypes.data, len(lst), limit, dst.ctypes.data, cap,
           mr.ctypes.data, out.ctypes.data)
    return n, dst[:max(n, 0)].tobytes(), mr[:len(lst)], out[0], dst[cap:]


def check_list(fn, src, lst, limit=0, cap=0, tag=""):
    n, got, mr, res, rest = run_list(fn, src, lst, limit, cap)
    emr, eres, eout = O.connection(src, lst, limit, 0, cap)
    assert res == eres, "%s: result %s, expected %s" % (tag, res, eres)
    assert n == len(eout) and got == eout, "%s: output differs (%d bytes, expected %d)" % (tag, n, len(eout))
    assert np.array_equal(mr, emr), "%s: message records %s, expected %s" % (tag, mr, emr)
    assert (rest == O.FILL).all(), tag + ": bytes behind the room written"
    return int(eres["status"])


def check_body(fn, body, tag, limit=0, cap=None):
    st, out = O.inflate_one(body, limit)
    return check_list(fn, np.frombuffer(body, np.uint8), [(0, len(body), O.RAW)], limit, len(out) if cap is None else cap, tag)


# ------------------------------------------------------------------ the rule vs zlib

def test_cases_are_what_they_say():
    """zlib gives stored, fixed and dynamic blocks where the table says so; the hand-built streams
    mean what their author meant; the skewed alphabet reaches 15-bit codes"""
    assert (IC.deflate(b"abc" * 50, 0)[0] >> 1) & 3 == 0
    assert (IC.deflate(b"abc" * 50, 6, 4)[0] >> 1) & 3 == 1          # Z_FIXED
    for lv in (1, 6, 9):
        assert (IC.deflate(IC.text(np.random.default_rng(lv), 400), lv)[0] >> 1) & 3 == 2
    assert O.inflate_one(bytes.fromhex("f248cdc9c90700")) == (O.OK, b"Hello")
    for name, body, meant in IC.hand_built():
        st, out = O.inflate_one(body)
        assert (st == O.ERR_DATA) == (meant is None), name
        assert meant is None or out == meant, name
    for body in (bytes.fromhex("0100000000"), bytes([7]), bytes.fromhex("0500fbff68690000")):
        assert O.inflate_one(body)[0] == O.ERR_DATA
    assert IC.max_code_length(IC.deflate(IC.skewed(), 6, 2)) == 15
    # the far match: distance symbol 29 with all 13 extra bits, its source the message's first byte,
    # in a message of at least 33 KiB; one literal fewer and the same match is one past the output
    far = IC.fixed_block_matches(IC.far_match())
    assert (32768, 10, 29, 8191, 32768) in far and max(m[4] for m in far) == 32768
    assert len(O.inflate_one(IC.far_match())[1]) >= 33 * 1024
    short = IC.fixed_block_matches(IC.far_match(1))
    assert (32767, 10, 29, 8191, 32768) in short and O.inflate_one(IC.far_match(1))[0] == O.ERR_DATA
    table = dict(IC.directed_table())
    assert table["distance 32768 from the first byte"] == IC.far_match()
    assert table["distance 32768 one past the output"] == IC.far_match(1)
    names = [n for n, _ in IC.directed_table()]
    assert len(names) == len(set(names)) >= 60


def test_directed_table(host):
    entry = entry_fn()
    seen = set()
    for name, body in IC.directed_table():
        for fn, what in ((host.ws_inflate_host_connection, "header"), (entry, "entry point")):
            seen.add(check_body(fn, body, "%s, %s" % (what, name)))
    assert seen == {O.OK, O.ERR_DATA}


def test_every_truncation_of_one_stream(host):
    prefixes = IC.truncations()
    assert len(prefixes) > 1400
    st = [check_body(host.ws_inflate_host_connection, b, "prefix %d" % len(b)) for b in prefixes]
    # the stream keeps its share of error prefixes (about a fifth, cuts inside its dynamic headers)
    assert st.count(O.ERR_DATA) == sum(O.inflate_one(b)[0] == O.ERR_DATA for b in prefixes)
    assert st.count(O.ERR_DATA) >= len(prefixes) // 8 and st.count(O.OK) >= len(prefixes) // 2


def test_every_single_bit_flip_of_a_dynamic_stream(host):
    st = [check_body(host.ws_inflate_host_connection, b, "flip %d" % k) for k, b in enumerate(IC.bit_flips())]
    assert st.count(O.ERR_DATA) >= 100 and st.count(O.OK) >= 100


def test_random_bodies_and_their_mutations(host):
    """20,000 bodies: none left out, every one either inflates to zlib's bytes or gets zlib's verdict"""
    bodies = IC.random_cases()
    assert len(bodies) >= 20000 and max(len(b) for b in bodies) > 50000
    seen = {O.OK: 0, O.ERR_DATA: 0}
    for k, b in enumerate(bodies):
        seen[check_body(host.ws_inflate_host_connection, b, "random %d" % k)] += 1
    print("random bodies:", seen)
    assert seen[O.OK] >= 5000 and seen[O.ERR_DATA] >= 1000


def test_limits_in_decode_order(host):
    """the limit and the room against the model at every interesting size, on good bodies and on
    one whose second half is corrupt: an error before the limit's crossing is ERR_DATA, behind it
    never seen; the room is judged last"""
    rng = np.random.default_rng(12)
    data = IC.text(rng, 3000)
    good = IC.deflate(data, 6)
    bad = IC.deflate(data[:2000], 6) + O.TAIL + bytes([7])         # 2000 good bytes, then a block of type 3
    assert O.inflate_one(bad)[0] == O.ERR_DATA
    # both orders; at 1999 zlib has room for 2000 bytes and so still reaches the bad block
    assert O.inflate_one(bad, 1998)[0] == O.ERR_TOO_BIG and O.inflate_one(bad, 1999)[0] == O.inflate_one(bad, 2000)[0] == O.ERR_DATA
    entry = entry_fn()
    seen = set()
    for body in (good, bad, IC.deflate(data, 0), IC.deflate(b"r" * 3000, 6)):
        for limit in (0, 1, 2, 257, 258, 259, 1000, 1998, 1999, 2000, 2001, 2999, 3000, 3001):
            for cap in (0, 1, 999, 1999, 2000, 2999, 3000, 3001):
                for fn in (host.ws_inflate_host_connection, entry):
                    seen.add(check_list(fn, np.frombuffer(body, np.uint8), [(0, len(body), O.RAW)], limit, cap,
                                        "limit %d room %d" % (limit, cap)))
    assert seen == {O.OK, O.ERR_DATA, O.ERR_TOO_BIG, O.ERR_OUT_SPACE}


def test_entry_point_on_lists(host):
    """lists with SKIPs, a range error, an unknown kind, failures first, in the middle and last"""
    rng = np.random.default_rng(3)
    bodies = [IC.deflate(IC.text(rng, n), 6) for n in (0, 1, 50, 700)] + [bytes([7])]
    src = np.frombuffer(b"".join(bodies), np.uint8)
    offs = np.cumsum([0] + [len(b) for b in bodies])
    e = [(int(offs[k]), len(bodies[k]), O.RAW) for k in range(5)]
    skip, far, kind = (0, 0, O.SKIP), (len(src) - 1, 2, O.RAW), (0, 1, 9)
    lists = [[], [skip], [e[3]], [e[0], e[1], e[2], e[3]], [skip, e[3], skip, e[2]], [e[4], e[3]], [e[3], e[4], e[2]],
             [e[2], e[3], e[4]], [far, e[1]], [e[2], far], [(1 << 63, 1 << 63, O.RAW)], [(len(src) + 9, 1 << 62, O.SKIP), e[2]],
             [kind, e[2]], [e[3], e[3], e[3]]]
    entry = entry_fn()
    seen = set()
    for k, lst in enumerate(lists):
        for limit, cap in ((0, 4000), (700, 4000), (699, 4000), (0, 1400), (0, 1399), (0, 0)):
            for fn in (host.ws_inflate_host_connection, entry):
                seen.add(check_list(fn, src, lst, limit, cap, "list %d limit %d room %d" % (k, limit, cap)))
    assert seen == {O.OK, O.ERR_DATA, O.ERR_TOO_BIG, O.ERR_OUT_SPACE, O.ERR_RANGE}
    out, mr, res = W.inflate_host(src, np.array([e[2] + (0,), skip + (0,)], W.INFLATE_MSG_DTYPE), 100)
    assert out == O.inflate_one(bodies[2])[1] and int(res["n_msgs"]) == 1 and [int(v) for v in mr["out_off"]] == [0, 50]


# ------------------------------------------------------------------ the stand-alone program

def test_host_program_under_sanitizers(tmp_path):
    """the same source as a program of its own, built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as its own process over the directed table, the flips and a
    few thousand mutated bodies: source and destination are exactly as long as they are said to be"""
    exe = str(tmp_path / "inflate_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DINFLATE_HOST_MAIN", SRC, "-o", exe], check=True)
    bodies = [b for _, b in IC.directed_table()] + IC.bit_flips() + IC.truncations()[::5] + IC.random_cases(700, seed=77)
    blobs = []
    for k, body in enumerate(bodies):
        limit = 0 if k % 3 else 200
        st, out = O.inflate_one(body, limit)
        cap = len(out) if k % 5 else max(0, len(out) - 1)
        if st == O.OK and len(out) > cap:
            st, out = O.ERR_OUT_SPACE, b""
        blobs.append(struct.pack("<5I", len(body), limit, cap, st, len(out)) + body + out)
    with open(str(tmp_path / "cases.bin"), "wb") as f:
        f.write(struct.pack("<I", len(blobs)) + b"".join(blobs))
    assert len(blobs) >= 3000
    out = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("inflate_host ok: %d cases" % len(blobs)), out.stdout + out.stderr


# ------------------------------------------------------------------ ABI, arguments

def test_deflate_library_exports():
    """libwsframe_amd_deflate.so's symbol table is libwsframe_amd_cli.so's plus exactly the names
    wsframe_amd_deflate.h marks; the older libraries export none of them"""
    text = open(os.path.join(_lib.REPO, "include", "wsframe_amd_deflate.h")).read()
    marked = set(re.findall(r"WSFRAME_AMD_DEFLATE_EXPORT[^;]*?\b(websocketframe\w+)\s*\(", text, re.S))
    assert marked == set(_lib.DEFLATE_EXPORTS) and len(marked) == 3
    assert os.path.exists(_lib.DEFLATE_LIB_PATH), "libwsframe_amd_deflate.so is not built"
    assert dynamic_symbols(_lib.DEFLATE_LIB_PATH) == dynamic_symbols(_lib.CLI_LIB_PATH) | marked
    for path in (_lib.LIB_PATH, _lib.CTL_LIB_PATH, _lib.TEXT_LIB_PATH, _lib.PROTO_LIB_PATH, _lib.HS_LIB_PATH,
                 _lib.REPLY_LIB_PATH, _lib.SEND_LIB_PATH, _lib.CLI_LIB_PATH, _lib.BENCH_LIB_PATH):
        assert not dynamic_symbols(path) & marked, path


def test_constants_and_struct_layout(host, tmp_path):
    text = open(os.path.join(_lib.REPO, "include", "wsframe_amd_deflate.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"WEBSOCKET_INFLATE_(OK|ERR_\w+|NOT_RUN) = (\d+)", text)}
    assert enum == {"OK": 0, "ERR_DATA": 1, "ERR_TOO_BIG": 2, "ERR_OUT_SPACE": 3, "ERR_RANGE": 4, "NOT_RUN": 5}
    for name, value in enum.items():
        assert getattr(W, "INFLATE_" + name) == value == getattr(O, name)
    defs = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define WEBSOCKET_INFLATE_(\w+)\s+(\w+)", text)}
    assert defs == {"SKIP": 0xFFFFFFFF, "RAW": 1, "NONE": 0xFFFFFFFF}
    assert (W.INFLATE_SKIP, W.INFLATE_RAW, W.INFLATE_NONE) == (O.SKIP, O.RAW, O.NONE)
    assert (W.INFLATE_MSG_DTYPE, W.INFLATE_MSGRES_DTYPE, W.INFLATE_RES_DTYPE) == (O.MSG_DTYPE, O.MSGRES_DTYPE, O.RES_DTYPE)
    v = np.zeros(8, np.uint32)
    host.ws_inflate_host_sizes(v.ctypes.data)
    assert [int(x) for x in v] == [24, 8, 24, 8, 24, 8, 1856, 424]
    prog = tmp_path / "size.c"
    prog.write_text('#include "wsframe_amd_deflate.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu %zu %zu %zu %zu", '
                    "sizeof(WebsocketInflateMsg_t), sizeof(WebsocketInflateMsgRes_t), sizeof(WebsocketInflateResult_t), "
                    "offsetof(WebsocketInflateResult_t, first_bad), _Alignof(WebsocketInflateResult_t)); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(_lib.REPO, "include"), str(prog), "-o", exe],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "24 24 24 16 8"


def test_entry_point_refuses_bad_arguments():
    lib = _lib.load_deflate_lib()
    body = np.frombuffer(IC.deflate(b"Hello"), np.uint8)
    msg = np.zeros(1, O.MSG_DTYPE)
    msg[0] = (0, len(body), O.RAW, 0)
    dst = np.full(64, O.FILL, np.uint8)
    out = np.full(6, 7, np.uint32)

    def call(s=body.ctypes.data, n=len(body), m=msg.ctypes.data, flags=0, d=dst.ctypes.data, cap=64, o=out.ctypes.data):
        return lib.websocketframeInflateHost(s, n, m, 1, 0, flags, d, cap, None, o)
    for kw, word in ((dict(flags=1), b"flag"), (dict(s=None), b"NULL"), (dict(m=None), b"NULL"), (dict(o=None), b"NULL"),
                     (dict(d=None), b"NULL")):
        assert call(**kw) < 0 and word in lib.websocketframeGpuLastError(), kw
        assert (dst == O.FILL).all() and (out == 7).all()
    assert call() == 5 and dst[:5].tobytes() == b"Hello" and (dst[5:] == O.FILL).all()
    assert call(d=None, cap=0) == 0 and int(out.view(O.RES_DTYPE)[0]["status"]) == O.ERR_OUT_SPACE
