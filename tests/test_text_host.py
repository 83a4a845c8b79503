"""The text validator's rule (util_amd/csrc/ws_utf8.h: the look-back byte rule, the unfinished
tail, the state word) compiled for the host and held against the oracle (text_oracle.py), plus
the symbol table of libwsframe_amd_text.so. CPU only: g++, ctypes and numpy."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import text_oracle as T
from test_abi import dynamic_symbols
from util_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDARY = bytes([0x00, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED,
                  0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF])
PHASES = (-1, 0, 2, 13, 15)       # -1: byte by byte; else 16-B chunks with the body at that phase


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("utf8") / "libutf8_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "c", "utf8_host.cpp"),
                    "-o", so_path], check=True)
    lib = C.CDLL(so_path)
    lib.ws_utf8_host_text.restype = C.c_uint
    lib.ws_utf8_host_text.argtypes = [C.c_char_p, C.c_ulonglong, C.c_uint, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_uint)]
    lib.ws_utf8_host_all.restype = None
    lib.ws_utf8_host_all.argtypes = [C.c_char_p, C.c_uint, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def exhaustive(host, alphabet, length, phase):
    total = len(alphabet) ** length
    vc, vo = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
    st = np.zeros(total, np.uint32)
    host.ws_utf8_host_all(bytes(alphabet), len(alphabet), length, phase, vc.ctypes.data, vo.ctypes.data, st.ctypes.data)
    ec, eo, es = expected(bytes(alphabet), length)
    for got, exp, what in ((vc, ec, "complete"), (vo, eo, "open"), (st, es, "state")):
        bad = np.nonzero(got != exp)[0]
        if len(bad):
            s = bytes(list(itertools.product(alphabet, repeat=length))[bad[0]])
            raise AssertionError("%s of %s at phase %d: %x, oracle %x" % (what, s.hex(), phase, got[bad[0]], exp[bad[0]]))


_expected = {}


def expected(alphabet, length):
    """the oracle over every string of `length` bytes of the alphabet, computed once"""
    if (alphabet, length) not in _expected:
        ec, eo, es = [], [], []
        for s in itertools.product(alphabet, repeat=length):
            s = bytes(s)
            word = T.state_word(s)
            ec.append(T.VALID if T.complete_ok(s) else T.INVALID)
            eo.append(T.INVALID if word & T.ST_FAILED else T.VALID)
            es.append(word)                                # (FAILED is "not viable": state_word's first line)
        _expected[(alphabet, length)] = (np.array(ec, np.uint8), np.array(eo, np.uint8), np.array(es, np.uint32))
    return _expected[(alphabet, length)]


def test_oracle_viable_is_the_definition():
    """the oracle's cheap viable() equals the 40-decode definition: all strings of 1 and 2 bytes,
    and all of 3 over the boundary alphabet"""
    for n, alphabet in ((1, range(256)), (2, range(256)), (3, BOUNDARY)):
        for s in itertools.product(alphabet, repeat=n):
            assert T.viable(bytes(s)) == T.viable_literal(bytes(s)), bytes(s).hex()
    assert T.state_word(b"a\xe0\xa0") == T.ST_PENDING | 2 << 24 | 0xA0E0
    assert T.state_word(b"a\xe0\x80") == T.ST_PENDING | T.ST_FAILED


@pytest.mark.parametrize("length", [1, 2])
def test_every_short_string(host, length):
    """every string of 1 or 2 bytes over all 256 values"""
    for phase in (-1, 15):
        exhaustive(host, bytes(range(256)), length, phase)


@pytest.mark.parametrize("length", [3, 4])
def test_boundary_alphabet(host, length):
    """every string of 3 or 4 bytes over the lead / continuation range boundaries"""
    for phase in (-1, 14) if length == 4 else PHASES:
        exhaustive(host, BOUNDARY, length, phase)


def corpus():
    rng = np.random.default_rng(6455)
    cps = [0x24, 0x7F, 0x80, 0xA2, 0x7FF, 0x800, 0x20AC, 0xD7FF, 0xE000, 0xFFFD, 0xFFFF, 0x10000, 0x10348, 0x10FFFF]
    out = []
    for k in range(150):
        n = int(rng.integers(1, 24))
        s = "".join(chr(int(c)) for c in rng.choice(cps, n)).encode("utf-8")
        out.append(s)
        b = bytearray(s)
        kind = k % 3
        pos = int(rng.integers(0, len(b)))
        if kind == 0:
            b[pos] = int(rng.choice(list(BOUNDARY)))
        elif kind == 1:
            del b[pos]
        else:
            b.insert(pos, int(rng.choice(list(BOUNDARY))))
        out.append(bytes(b))
    return out


def run_split(host, s, cuts, complete, phase):
    """the message s in batches cut at `cuts`: every batch but the last leaves it open"""
    conn = T.TextConn()
    state = 0
    edges = [0] + list(cuts) + [len(s)]
    for j in range(len(edges) - 1):
        part = s[edges[j]:edges[j + 1]]
        last = j == len(edges) - 2
        done = 1 if (last and complete) else 0
        out = C.c_uint(0)
        v = host.ws_utf8_host_text(part, len(part), state, 1 if j else 0, done, phase, C.byref(out))
        ov, _fb, oword = conn.batch([(1, part, done, 1 if j else 0, 1)])
        what = "%s cuts %s batch %d complete %d phase %d" % (s.hex(), cuts, j, complete, phase)
        assert v == ov[0], what
        if not done:
            state = out.value
            assert state == oword, what + ": state %08x, oracle %08x" % (state, oword)


def test_every_split_into_two_and_three_batches(host):
    """a few hundred valid and corrupted strings, every split into two and (for the shorter
    ones) three batches, as complete and as open messages, state words included"""
    for idx, s in enumerate(corpus()):
        phase = PHASES[idx % len(PHASES)]
        for complete in (0, 1):
            for a in range(len(s) + 1):
                run_split(host, s, (a,), complete, phase)
            if len(s) <= 16:
                for a in range(len(s) + 1):
                    for b in range(a, len(s) + 1):
                        run_split(host, s, (a, b), complete, phase)


def test_text_library_exports():
    """libwsframe_amd_text.so's symbol table is libwsframe_amd_ctl.so's plus exactly the names
    wsframe_amd_text.h marks; the two older libraries do not export them"""
    src = open(os.path.join(_lib.REPO, "include", "wsframe_amd_text.h")).read()
    marked = set(re.findall(r"WSFRAME_AMD_TEXT_EXPORT[^;]*?\b(websocketframe\w+)\s*\(", src, re.S))
    assert marked == set(_lib.TEXT_EXPORTS) and len(marked) == 1
    assert os.path.exists(_lib.TEXT_LIB_PATH), "libwsframe_amd_text.so is not built"
    assert dynamic_symbols(_lib.TEXT_LIB_PATH) == dynamic_symbols(_lib.CTL_LIB_PATH) | marked
    assert not dynamic_symbols(_lib.LIB_PATH) & marked
    assert not dynamic_symbols(_lib.CTL_LIB_PATH) & marked
