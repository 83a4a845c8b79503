"""The protocol check's rule (util_amd/csrc/ws_proto.h: a frame's code, the run summary and its
combine, the state word) compiled for the host and held against the sequential oracle
(proto_oracle.py), the exported host step held against the same sweep, the symbol table of
libwsframe_amd_proto.so, the directed table against the oracle, and the coverage the GPU suite's
seeded random cases reach. CPU only: g++, ctypes and numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import proto_cases as PC
import proto_oracle as P
from test_abi import dynamic_symbols
from util_amd import _lib
from util_amd import wsframe as W

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "proto_host.cpp")
LIMIT = 100
STATES = [0, P.ST_OPEN, P.ST_OPEN | (LIMIT - 1), P.ST_OPEN | LIMIT, P.ST_OPEN | (LIMIT + 1), P.ST_CLOSED]
FLAGS = [e | w for e in (0, P.EXPECT_MASKED, P.EXPECT_UNMASKED) for w in (0, P.WIRE_MASKED)]
RSV = [0, 0x40, 0x70]
DATALEN = [0, 1, 2, 125, 126]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("proto") / "libproto_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so_path], check=True)
    lib = C.CDLL(so_path)
    vp, u32, u64 = C.c_void_p, C.c_uint, C.c_ulonglong
    lib.ws_proto_host_steps.restype = None
    lib.ws_proto_host_steps.argtypes = [u32, vp, vp, vp, vp, vp, u32, u32, u64, vp, vp]
    lib.ws_proto_host_fold_all.restype = u64
    lib.ws_proto_host_fold_all.argtypes = [u32]
    lib.ws_proto_host_fold_random.restype = u64
    lib.ws_proto_host_fold_random.argtypes = [u64, u32, u32]
    return lib


def sweep_inputs():
    """(state, b0, masked, datalen, close code) rows: every first byte, both mask bits, the
    lengths and the states with one valid and one invalid CLOSE code; then every CLOSE code
    0..5100 on a CLOSE of 2 bytes from each state"""
    rows = [(st, b0, m, n, code) for st in STATES for b0 in range(256) for m in (0, 1) for n in DATALEN
            for code in ((1000, 1005) if b0 & 15 == 8 and n >= 2 else (0,))]
    rows += [(st, 0x88, 1, 2, code) for st in (0, P.ST_OPEN | 5, P.ST_CLOSED) for code in range(5101)]
    return rows


_oracle = {}


def oracle_sweep(flags, rsv_allowed):
    """the oracle's (code, state) of every row, computed once per setting"""
    if (flags, rsv_allowed) not in _oracle:
        out = []
        for st, b0, m, n, code in sweep_inputs():
            conn = P.Conn(st)
            c = conn.frame(b0, b0 & 15, b0 >> 7, m, n, [code >> 8, code & 0xFF], flags, rsv_allowed, LIMIT)
            out.append((c, conn.word()))
        _oracle[(flags, rsv_allowed)] = out
    return _oracle[(flags, rsv_allowed)]


SETTINGS = [(f, r) for f in FLAGS for r in RSV]              # each flag combination with each rsv_allowed


@pytest.fixture(scope="module")
def sweep_arrays():
    rows = sweep_inputs()
    return (np.array([r[0] for r in rows], np.uint64), np.array([r[1] for r in rows], np.uint8),
            np.array([r[2] for r in rows], np.uint8), np.array([r[3] for r in rows], np.uint64),
            np.array([r[4] for r in rows], np.uint16))


@pytest.mark.parametrize("flags,rsv", SETTINGS)
def test_header_step_matches_the_oracle(host, sweep_arrays, flags, rsv):
    rows = sweep_inputs()
    st, b0, m, n, cc = sweep_arrays
    code = np.zeros(len(rows), np.uint8)
    out = np.zeros(len(rows), np.uint64)
    host.ws_proto_host_steps(len(rows), st.ctypes.data, b0.ctypes.data, m.ctypes.data, n.ctypes.data, cc.ctypes.data,
                             flags, rsv, LIMIT, code.ctypes.data, out.ctypes.data)
    for i, (oc, ow) in enumerate(oracle_sweep(flags, rsv)):
        assert (int(code[i]), int(out[i])) == (oc, ow), \
            "row %s flags %d rsv %#x: header (%d, %x), oracle (%d, %x)" % (rows[i], flags, rsv, code[i], out[i], oc, ow)


@pytest.mark.parametrize("flags,rsv", SETTINGS)
def test_exported_host_step_matches_the_oracle(flags, rsv):
    """websocketframeProtoStepHost through ctypes: every row of the same sweep"""
    step = _lib.load_proto_lib().websocketframeProtoStepHost
    st = C.c_ulonglong(0)
    ref = C.byref(st)
    exp = oracle_sweep(flags, rsv)
    for i, (s0, b0, m, n, code) in enumerate(sweep_inputs()):
        st.value = s0
        got = step(ref, b0, m, n, code.to_bytes(2, "big"), flags, rsv, LIMIT)
        assert (got, st.value) == exp[i], "row %s flags %d rsv %#x: %s, oracle %s" % (
            (s0, b0, m, n, code), flags, rsv, (got, st.value), exp[i])


def test_exported_host_step_refuses_bad_arguments():
    lib = _lib.load_proto_lib()
    st = C.c_ulonglong(P.ST_OPEN | 3)
    for flags, rsv in ((8, 0), (P.EXPECT_MASKED | P.EXPECT_UNMASKED, 0), (0, 0x80), (0, 0x0F)):
        assert lib.websocketframeProtoStepHost(C.byref(st), 0x81, 1, 1, None, flags, rsv, 0) < 0
        assert st.value == P.ST_OPEN | 3 and lib.websocketframeGpuLastError() != b""
    assert W.proto_step_host(0, 0x01, 1, 5) == (0, P.ST_OPEN | 5)


def test_summary_fold_equals_the_step(host):
    """every cut of a sequence into tiles, folded with the header's combine, gives the sequential
    step's codes and state: all sequences of up to 6 of 6 symbols, 10,000 random ones of 12"""
    assert host.ws_proto_host_fold_all(6) == 0


def test_summary_fold_equals_the_step_random(host):
    assert host.ws_proto_host_fold_random(6455, 10000, 12) == 0


def test_host_program_runs_standalone(tmp_path):
    """the same source as a program of its own (the form a sanitizer build takes): a tenth of the folds"""
    exe = str(tmp_path / "proto_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-DPROTO_HOST_MAIN", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "proto_host ok", out.stdout + out.stderr


def test_proto_library_exports():
    """libwsframe_amd_proto.so's symbol table is libwsframe_amd_text.so's plus exactly the names
    wsframe_amd_proto.h marks; the four older libraries export none of them"""
    src = open(os.path.join(_lib.REPO, "include", "wsframe_amd_proto.h")).read()
    marked = set(re.findall(r"WSFRAME_AMD_PROTO_EXPORT[^;]*?\b(websocketframe\w+)\s*\(", src, re.S))
    assert marked == set(_lib.PROTO_EXPORTS) and len(marked) == 2
    assert os.path.exists(_lib.PROTO_LIB_PATH), "libwsframe_amd_proto.so is not built"
    assert dynamic_symbols(_lib.PROTO_LIB_PATH) == dynamic_symbols(_lib.TEXT_LIB_PATH) | marked
    for path in (_lib.LIB_PATH, _lib.CTL_LIB_PATH, _lib.TEXT_LIB_PATH, _lib.BENCH_LIB_PATH):
        assert not dynamic_symbols(path) & marked, path


def test_constants_agree():
    """the header's enum, wsframe.py's constants and the oracle's"""
    src = open(os.path.join(_lib.REPO, "include", "wsframe_amd_proto.h")).read()
    enum = {k: int(v, 0) for k, v in re.findall(r"WEBSOCKET_PROTO_(\w+) = (\w+)", src)}
    for name, value in enum.items():
        assert getattr(W, "PROTO_" + name) == value == getattr(P, name), name
    assert len(enum) == 13
    for name in ("EXPECT_MASKED", "EXPECT_UNMASKED", "WIRE_MASKED", "NONE", "ST_OPEN", "ST_CLOSED"):
        assert getattr(W, "PROTO_" + name) == getattr(P, name)
    assert W.PROTO_RES_DTYPE == P.RES_DTYPE


def test_directed_table_agrees_with_the_oracle():
    """the hand-written codes of the directed table are what the oracle says, on the decoded and
    on the still-masked wire"""
    for name, frames, flags, rsv, codes, first_bad, code, status, close_frame in PC.directed_table():
        b = PC.Batch([frames], len(frames) + 1)
        for fl in (flags, flags | P.WIRE_MASKED):
            oc, ores, _ = b.expect(fl, rsv)
            assert list(oc[:len(codes)]) == codes, name
            assert tuple(int(v) for v in ores[0]) == (first_bad, code, status, close_frame), name


def test_oracle_carries_across_batches():
    """the oracle over a connection cut in two equals the oracle over it whole (its own sanity:
    the GPU's carry test leans on it)"""
    frames = PC.carry_script()
    whole = PC.Batch([frames], len(frames))
    wc, wr, ww = whole.expect(P.EXPECT_MASKED, 0, 6, np.zeros(1, np.uint64))
    for cut in range(len(frames) + 1):
        a, b = PC.Batch([frames[:cut]], len(frames)), PC.Batch([frames[cut:]], len(frames))
        ac, _, aw = a.expect(P.EXPECT_MASKED, 0, 6, np.zeros(1, np.uint64))
        bc, _, bw = b.expect(P.EXPECT_MASKED, 0, 6, aw)
        assert list(ac[:cut]) + list(bc[:len(frames) - cut]) == list(wc[:len(frames)]) and bw[0] == ww[0], cut


def test_random_cases_cover_every_code_and_position():
    """The GPU suite's seeded random cases (same builders, same seed), on the oracle alone: every
    error code is some segment's first_bad at least 20 times; every code shows, as a frame's code
    and as a segment's first_bad, at frame 0, inside a tile, on a tile's last frame, on a tile's
    first (k > 0) and on a segment's last frame; AFTER_CLOSE and NOT_CONSUMED show at least 20
    times each. A tile's last and first frame are those at list positions (the batch's frames laid
    end to end, as the kernels cut them) 255 and 0 mod 256; the eight long segments stand alone in
    their batches, where that is k % 256 == 255 and k % 256 == 0."""
    cases = PC.random_cases()
    lens = sorted(int(n) for b, *_ in cases for n in b.res["n_frames"])
    assert len(lens) == 1008 and lens[0] >= 1 and lens[999] <= 40 and 200 <= lens[1000] and lens[-1] <= 1100
    assert all(b.nseg == 1 for b, *_ in cases[10:])
    first, where, where_first, after, notc = PC.coverage(cases)
    assert all(n >= 20 for n in first.values()), first
    for code in range(1, 11):
        assert where[code] == PC.CLASSES, (code, where[code])
        assert where_first[code] == PC.CLASSES, (code, where_first[code])
    assert after >= 20 and notc >= 20, (after, notc)
    drawn = {f & 3 for _b, f, *_ in cases}, {r for _b, _f, r, *_ in cases}
    assert drawn == ({0, P.EXPECT_MASKED, P.EXPECT_UNMASKED}, {0, 0x40, 0x70}), drawn
