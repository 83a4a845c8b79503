"""The handshake's rule (util_amd/csrc/ws_handshake.h) compiled for the host and the exported host
entry point (websocketframeHandshakeHost) held against the reference's recorded results
(tests/golden/handshake_batch.json) and, on the seeded random requests of the GPU suite, against
the host symbols of libwsframe_amd.so (pinned to the reference by tests/golden/handshake.json)
and the reference's own build where it is present; the symbol table of libwsframe_amd_hs.so; the
coverage the seeded requests reach; a stand-alone sanitizer build. CPU only: g++, ctypes, numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import handshake_cases as HC
from test_abi import dynamic_symbols
from util_amd import _lib
from util_amd import wsframe as W

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "handshake_host.cpp")


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("hs") / "libhs_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so_path], check=True)
    lib = C.CDLL(so_path)
    vp, u32, u64 = C.c_void_p, C.c_uint, C.c_ulonglong
    lib.ws_hs_host_one.restype = None
    lib.ws_hs_host_one.argtypes = [vp, u64, u32, vp, vp, vp, u32]
    lib.ws_hs_host_accept.restype = None
    lib.ws_hs_host_accept.argtypes = [vp, u32, vp]
    return lib


@pytest.fixture(scope="module")
def fixture_cases(golden):
    rows = golden("handshake_batch.json")
    table = HC.directed_table()
    assert [r["name"] for r in rows] == [n for n, _ in table], "regenerate tests/golden/handshake_batch.json"
    out = []
    for r, (_name, data) in zip(rows, table):
        assert bytes.fromhex(r["input"]) == data, r["name"]
        out.append((r["name"], data, {
            "ret": r["ret"], "key_off": r["key_off"], "key_len": r["key_len"],
            "proto_off": HC.NONE if r["proto_off"] is None else r["proto_off"], "proto_len": r["proto_len"],
            "accept": r["accept"].encode(), "resp": bytes.fromhex(r["resp"]), "resp_echo": bytes.fromhex(r["resp_echo"])}))
    return out


@pytest.fixture(scope="module")
def random_cases():
    reqs = HC.random_requests()
    lib = HC.host_symbols()
    exps = [HC.expected(lib, d) for d in reqs]
    return reqs, exps


def run_one(call, data, flags, resp_cap=4096, want_accept=True, want_resp=True):
    """(record tuple, accept 32 bytes, response buffer) of one request through `call`"""
    buf = np.full(len(data) + HC.PAD, 0xEE, np.uint8)
    buf[:len(data)] = np.frombuffer(data, np.uint8)
    hs = np.zeros(1, W.HS_DTYPE)
    acc = np.full(32, 0x5A, np.uint8)
    resp = np.full(resp_cap + 16, 0x77, np.uint8)
    call(buf.ctypes.data, len(data), flags, hs.ctypes.data, acc.ctypes.data if want_accept else None,
         resp.ctypes.data if want_resp else None, resp_cap)
    return tuple(int(v) for v in hs[0]), acc, resp


def check_against(call, name, data, exp):
    for flags in (0, HC.ECHO):
        want = exp["resp_echo"] if flags else exp["resp"]
        rec, acc, resp = run_one(call, data, flags)
        assert rec == HC.expected_record(exp, flags, True, 4096), (name, flags)
        if exp["ret"] > 0:
            assert bytes(acc) == exp["accept"] + b"\0\0\0\0", name
            assert bytes(resp[:len(want)]) == want and (resp[len(want):] == 0x77).all(), (name, flags)
        else:
            assert (acc == 0x5A).all() and (resp == 0x77).all(), name


def header_call(header):
    return lambda b, n, f, h, a, r, cap: header.ws_hs_host_one(b, n, f, h, a, r, cap)


def export_call():
    fn = _lib.load_hs_lib().websocketframeHandshakeHost

    def call(b, n, f, h, a, r, cap):
        assert fn(b, n, f, h, a, r, cap) == 0
    return call


def test_fixture_is_the_host_symbols_too(fixture_cases):
    """what the reference recorded is what libwsframe_amd.so's four symbols give (the seeded sweep
    leans on them)"""
    lib = HC.host_symbols()
    for name, data, exp in fixture_cases:
        assert HC.expected(lib, data) == exp, name


def test_header_matches_the_fixture(header, fixture_cases):
    for name, data, exp in fixture_cases:
        check_against(header_call(header), name, data, exp)


def test_exported_host_entry_matches_the_fixture(fixture_cases):
    call = export_call()
    for name, data, exp in fixture_cases:
        check_against(call, name, data, exp)


def test_header_matches_the_host_symbols_on_the_seeded_sweep(header, random_cases):
    reqs, exps = random_cases
    for i, (d, x) in enumerate(zip(reqs, exps)):
        check_against(header_call(header), "random %d" % i, d, x)


def test_exported_host_entry_matches_the_seeded_sweep(random_cases):
    reqs, exps = random_cases
    call = export_call()
    for i, (d, x) in enumerate(zip(reqs[::4], exps[::4])):
        check_against(call, "random %d" % (4 * i), d, x)


def test_seeded_sweep_agrees_with_the_reference_build(random_cases):
    """where the reference's own build is present, the seeded requests' expectations are its too"""
    ref = HC.reference_lib()
    if ref is None:
        return
    reqs, exps = random_cases
    for i, (d, x) in enumerate(zip(reqs, exps)):
        assert HC.expected(ref, d) == x, i


def test_seeded_sweep_covers_every_class(random_cases):
    """each class of result is at least 5 % of the seeded requests, on the reference symbols' own
    results: a degenerate generator cannot pass quietly"""
    reqs, exps = random_cases
    assert len(reqs) == 4096 and min(map(len, reqs)) >= 20 and max(map(len, reqs)) <= 3000
    cov = HC.coverage(reqs, exps)
    assert all(v >= 0.05 for v in cov.values()), cov
    assert len({len(r) // 1024 for r in reqs}) == 3          # one, two and three rounds of the parse kernel


def test_accept_for_every_key_length(header):
    """SHA-1's padding at every position: keys of 0..200 bytes against websocketframeComputeSecAccept"""
    for n in range(201):
        key = HC.filler(n, n)
        kb = np.frombuffer(key + b"\0", np.uint8).copy()
        out = np.zeros(32, np.uint8)
        header.ws_hs_host_accept(kb.ctypes.data, n, out.ctypes.data)
        assert bytes(out[:28]).decode() == W.websocketframeComputeSecAccept(key), n
        assert not out[28:].any()


def test_capacity_and_optional_outputs(fixture_cases):
    call = export_call()
    by_name = {n: (d, x) for n, d, x in fixture_cases}
    data, exp = by_name["with protocol"]
    for flags, want in ((0, exp["resp"]), (HC.ECHO, exp["resp_echo"])):
        for cap, fl in ((len(want) - 1, W.HS_RESP_NO_SPACE), (len(want), W.HS_RESP_WRITTEN), (len(want) + 1, W.HS_RESP_WRITTEN)):
            rec, _acc, resp = run_one(call, data, flags, resp_cap=cap)
            assert rec == HC.expected_record(exp, flags, True, cap) and rec[6] == fl and rec[5] == len(want)
            if fl == W.HS_RESP_WRITTEN:
                assert bytes(resp[:len(want)]) == want and (resp[len(want):] == 0x77).all()
            else:
                assert (resp == 0x77).all()
    rec, acc, resp = run_one(call, data, HC.ECHO, want_resp=False)
    assert rec == HC.expected_record(exp, HC.ECHO, False, 0) and rec[6] == 0 and (resp == 0x77).all()
    assert bytes(acc[:28]) == exp["accept"]
    rec, acc, resp = run_one(call, data, 0, want_accept=False)
    assert rec[6] == W.HS_RESP_WRITTEN and (acc == 0x5A).all() and bytes(resp[:129]) == exp["resp"]
    d, a, r = W.handshake_host(data, W.HS_ECHO_PROTOCOL)
    assert (int(d["ret"]), a, r) == (exp["ret"], exp["accept"], exp["resp_echo"])


def test_exported_host_entry_refuses_bad_arguments():
    lib = _lib.load_hs_lib()
    hs = np.full(1, 7, np.uint32).repeat(8)
    buf = np.zeros(64, np.uint8)
    for flags in (2, 4, 0x80000000):
        assert lib.websocketframeHandshakeHost(buf.ctypes.data, 10, flags, hs.ctypes.data, None, None, 0) < 0
        assert (hs == 7).all() and lib.websocketframeGpuLastError() != b""
    assert lib.websocketframeHandshakeHost(buf.ctypes.data, 10, 0, None, None, None, 0) < 0
    # a length the reference's int return cannot express: flagged, never read
    assert lib.websocketframeHandshakeHost(buf.ctypes.data, 1 << 31, 0, hs.ctypes.data, None, None, 0) == 0
    rec = hs.view(W.HS_DTYPE)[0]
    assert (int(rec["ret"]), int(rec["flags"]), int(rec["proto_off"])) == (-1, W.HS_ERR_SEG_LEN, W.HS_NONE)


def test_hs_library_exports():
    """libwsframe_amd_hs.so's symbol table is libwsframe_amd_proto.so's plus exactly the names
    wsframe_amd_handshake.h marks; the older libraries export none of them"""
    src = open(os.path.join(_lib.REPO, "include", "wsframe_amd_handshake.h")).read()
    marked = set(re.findall(r"WSFRAME_AMD_HS_EXPORT[^;]*?\b(websocketframe\w+)\s*\(", src, re.S))
    assert marked == set(_lib.HS_EXPORTS) and len(marked) == 2
    assert os.path.exists(_lib.HS_LIB_PATH), "libwsframe_amd_hs.so is not built"
    assert dynamic_symbols(_lib.HS_LIB_PATH) == dynamic_symbols(_lib.PROTO_LIB_PATH) | marked
    for path in (_lib.LIB_PATH, _lib.CTL_LIB_PATH, _lib.TEXT_LIB_PATH, _lib.PROTO_LIB_PATH, _lib.BENCH_LIB_PATH):
        assert not dynamic_symbols(path) & marked, path


def test_constants_agree():
    src = open(os.path.join(_lib.REPO, "include", "wsframe_amd_handshake.h")).read()
    consts = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define WEBSOCKET_HS_(\w+)\s+(\w+)", src)}
    assert consts == {"NONE": W.HS_NONE, "RESP_WRITTEN": W.HS_RESP_WRITTEN, "RESP_NO_SPACE": W.HS_RESP_NO_SPACE,
                      "ERR_SEG_LEN": W.HS_ERR_SEG_LEN, "ECHO_PROTOCOL": W.HS_ECHO_PROTOCOL}
    assert (HC.NONE, HC.ECHO, HC.PAD) == (W.HS_NONE, W.HS_ECHO_PROTOCOL, W.BATCH_PAD)
    fields = re.search(r"typedef struct WebsocketHandshakeDesc_t \{(.*?)\} WebsocketHandshakeDesc_t;", src, re.S).group(1)
    names = re.findall(r"^\s*(?:unsigned )?int (\w+);", fields, re.M)
    assert tuple(names) == W.HS_DTYPE.names


def test_sanitizer_program_on_the_directed_table(tmp_path, fixture_cases):
    """the same source as a program of its own under AddressSanitizer and UBSan, run with no
    preload: every directed case from a heap buffer of exactly len + 32 bytes into response buffers
    of exactly resp_len bytes (and one byte less: nothing written)"""
    exe = str(tmp_path / "handshake_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DHS_HOST_MAIN", SRC, "-o", exe],
                   check=True)
    path = str(tmp_path / "cases.txt")

    def hx(b):
        return b.hex() if b else "-"
    with open(path, "w") as f:
        for _name, data, x in fixture_cases:
            f.write("%s %d %d %d %d %d %s %s %s\n" % (hx(data), x["ret"], x["key_off"], x["key_len"], x["proto_off"],
                                                      x["proto_len"], hx(x["accept"]), hx(x["resp"]), hx(x["resp_echo"])))
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "handshake_host ok %d" % len(fixture_cases), out.stdout + out.stderr
