"""The client handshake's rule (util_amd/csrc/ws_client.h) compiled for the host and the exported
host entry points (websocketframeClientRequestHost, websocketframeClientVerifyHost) held against
the model of tests/client_oracle.py: requests against the two templates of include/wsframe_amd.h
and through the reference-pinned server side, the directed verify table, the seeded sweep and its
coverage; bad arguments, constants, the symbol table of libwsframe_amd_cli.so; a stand-alone
sanitizer build. CPU only: g++, ctypes, numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import client_cases as CC
import client_oracle as CO
import handshake_cases as HC
from test_abi import dynamic_symbols
from util_amd import _lib
from util_amd import wsframe as W

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "client_host.cpp")
HEADER = os.path.join(_lib.REPO, "include", "wsframe_amd_client.h")


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("cli") / "libcli_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", so_path], check=True)
    lib = C.CDLL(so_path)
    vp, u32, u64 = C.c_void_p, C.c_uint, C.c_ulonglong
    lib.ws_cl_host_verify.restype = None
    lib.ws_cl_host_verify.argtypes = [vp, u64, vp, vp, u32, u32, vp]
    lib.ws_cl_host_request.restype = None
    lib.ws_cl_host_request.argtypes = [vp, u32, vp, u32, vp, u32, vp, vp, u32, vp, vp]
    return lib


@pytest.fixture(scope="module")
def templates():
    """the two request templates, parsed out of include/wsframe_amd.h's macros"""
    src = open(os.path.join(_lib.REPO, "include", "wsframe_amd.h")).read()
    out = []
    for name in ("WEBSOCKET_SIMPLE_HTTP_HANDSHAKE_REQUEST_FMT", "WEBSOCKET_SIMPLE_HTTP_HANDSHAKE_REQUEST_WITH_PROTOCOL_FMT"):
        body = re.search(r"#define %s\b(.*?)\n\s*\n" % name, src, re.S).group(1)
        text = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', body))
        out.append(text.encode().decode("unicode_escape").encode("latin-1"))
    assert out[0].count(b"%s") == 2 and out[1].count(b"%s") == 3 and out[0].endswith(b"\r\n\r\n")
    return out


@pytest.fixture(scope="module")
def sweep():
    cases = CC.random_responses()
    return cases, [CO.verify(d, CC.EXPECT, off, mh) for d, off, mh in cases]


def arr(b):
    return np.frombuffer(bytes(b) + b"\0", np.uint8).copy()


def verify_header(header, data, expect, offered, max_head):
    buf = np.full(len(data) + CO.PAD, 0xEE, np.uint8)
    buf[:len(data)] = np.frombuffer(data, np.uint8)
    cv = np.full(1, 7, np.uint32).repeat(8)
    ex, of = arr(expect), arr(offered)
    header.ws_cl_host_verify(buf.ctypes.data, len(data), ex.ctypes.data, of.ctypes.data if offered else None, len(offered),
                             max_head, cv.ctypes.data)
    return tuple(int(v) for v in cv.view(W.CLI_VERIFY_DTYPE)[0])


def verify_export(data, expect, offered, max_head):
    return tuple(int(v) for v in W.client_verify_host(data, expect, offered, max_head))


def request_header(header, path, nonce, proto=b"", host=b"", cap=4096, want_req=True):
    a = [arr(x) for x in (path, proto, host, nonce)]
    req = np.full(cap + 16, 0x77, np.uint8)
    expect = np.full(32, 0x5A, np.uint8)
    rd = np.full(4, 7, np.uint32)
    header.ws_cl_host_request(a[0].ctypes.data, len(path), a[1].ctypes.data, len(proto), a[2].ctypes.data, len(host),
                              a[3].ctypes.data, req.ctypes.data if want_req else None, cap, expect.ctypes.data, rd.ctypes.data)
    return tuple(int(v) for v in rd), req, expect


def nonce_of(i):
    return bytes((i * 37 + k * 11 + (i >> 3)) & 0xFF for k in range(16))


# ------------------------------------------------------------------ requests

def test_model_request_is_the_template(templates):
    """the model's written-out text is the header's two templates filled by %"""
    for proto in (b"", b"chat, superchat"):
        assert CO.request(b"/chat", CC.NONCE, proto) == CO.request(b"/chat", CC.NONCE, proto, templates=templates)


def test_request_equals_the_template(header, templates):
    """paths of 1..300 bytes, with and without a protocol: exactly the template filled by Python's %;
    the Host variant inserts exactly one line"""
    for n in range(1, 301):
        path = b"/" + HC.filler(n - 1, n)
        for proto in (b"", b"p%d, chat" % n):
            nonce = nonce_of(n)
            want = templates[1] % (path, CO.key_of(nonce), proto) if proto else templates[0] % (path, CO.key_of(nonce))
            rec, req, expect = request_header(header, path, nonce, proto)
            assert rec == (len(want), want.index(CO.key_of(nonce)), W.CLI_REQ_WRITTEN, 0), n
            assert bytes(req[:len(want)]) == want and (req[len(want):] == 0x77).all(), n
            assert bytes(expect) == CO.expect_of(nonce), n
            d, r, e = W.client_request_host(path, nonce, proto)
            assert (tuple(int(v) for v in d), r, e) == (rec, want, CO.expect_of(nonce)), n
            if n % 7 == 0:
                host = b"h%d.example.com:8080" % n
                rec, req, _e = request_header(header, path, nonce, proto, host)
                line, rest = want.split(b"\r\n", 1)
                with_host = line + b"\r\nHost: " + host + b"\r\n" + rest
                assert rec == (len(with_host), with_host.index(CO.key_of(nonce)), W.CLI_REQ_WRITTEN, 0)
                assert bytes(req[:len(with_host)]) == with_host and (req[len(with_host):] == 0x77).all()
                assert W.client_request_host(path, nonce, proto, host)[1] == with_host == CO.request(path, nonce, proto, host)


def test_request_errors_and_capacity(header):
    nonce = nonce_of(5)
    ok = CO.request(b"/a", nonce, b"chat", b"h")
    for cap, fl in ((len(ok) - 1, W.CLI_REQ_NO_SPACE), (len(ok), W.CLI_REQ_WRITTEN), (len(ok) + 1, W.CLI_REQ_WRITTEN)):
        rec, req, expect = request_header(header, b"/a", nonce, b"chat", b"h", cap)
        assert rec == CO.request_record(b"/a", nonce, b"chat", b"h", cap)[0] and rec[2] == fl
        assert bytes(expect) == CO.expect_of(nonce)
        assert (req == 0x77).all() if fl == W.CLI_REQ_NO_SPACE else bytes(req[:len(ok)]) == ok and (req[len(ok):] == 0x77).all()
    rec, req, expect = request_header(header, b"/a", nonce, want_req=False)
    assert rec == CO.request_record(b"/a", nonce)[0] and rec[2] == 0 and (req == 0x77).all()
    assert bytes(expect) == CO.expect_of(nonce)
    bad = [(b"", b"", b""), (b"/a b", b"", b""), (b"/a\r\nX: y", b"", b""), (b"/\x7f", b"", b""), (b"/\x00", b"", b""),
           (b"/a", b"chat\r\nX: y", b""), (b"/a", b"a\tb", b""), (b"/a", b"", b"h\n"), (b"/a", b"", b"h\x7f"), (b"", b"\n", b"")]
    for path, proto, host in bad:
        want = CO.request_record(path, nonce, proto, host, 4096)
        assert want[0][2] & (W.CLI_ERR_RANGE | W.CLI_ERR_BYTES)
        rec, req, expect = request_header(header, path, nonce, proto, host)
        assert rec == want[0] and (req == 0x77).all() and (expect == 0x5A).all(), (path, proto, host)
        d, r, e = W.client_request_host(path, nonce, proto, host)
        assert (tuple(int(v) for v in d), r, e) == (want[0], None, None)
    # what the two byte rules let through: a space and bytes >= 0x80 in host and protocol, >= 0x80 in the path
    for path, proto, host in ((b"/\x80\xff", b"a b\xc3\xa9", b"h \xfe"),):
        rec, req, _e = request_header(header, path, nonce, proto, host)
        want = CO.request(path, nonce, proto, host)
        assert rec[2] == W.CLI_REQ_WRITTEN and bytes(req[:len(want)]) == want


def test_round_trip_through_the_pinned_server_side(header):
    """every built request fed to websocketframeHandshakeHost (pinned to the reference): ret is
    req_len, the key range lies at key_off, its accept is d_expect, and its written responses,
    plain and echoed, verify with the right proto_off; the reference's own build where present"""
    ref = HC.reference_lib()
    for i in range(64):
        nonce = nonce_of(i)
        path = b"/" + HC.filler(i * 5 % 90, i)
        proto = (b"", b"chat", b"a, bb ,ccc")[i % 3]
        host = b"example.com" if i % 4 == 0 else b""
        rec, req, expect = request_header(header, path, nonce, proto, host)
        data = bytes(req[:rec[0]])
        for flags in (0, W.HS_ECHO_PROTOCOL):
            hs, acc, resp = W.handshake_host(data, flags)
            assert int(hs["ret"]) == rec[0] and (int(hs["key_off"]), int(hs["key_len"])) == (rec[1], 24), i
            assert acc + b"\0\0\0\0" == bytes(expect) == CO.expect_of(nonce), i
            echoed = flags and proto
            if echoed and b"," in proto:
                # the server echoes the whole offered list: not an element, the client must fail it
                want = (-1, CO.PROTOCOL)
            else:
                want = (len(resp), 0)
            for got in (verify_header(header, resp, bytes(expect), proto, 0), verify_export(resp, bytes(expect), proto, 0)):
                assert got == CO.verify(resp, bytes(expect), proto, 0) and got[:2] == want, (i, flags)
                if echoed and want[0] > 0:
                    assert resp[got[3]:got[3] + got[4]] == proto
                else:
                    assert got[3] == CO.NONE
        if ref is not None:
            x = HC.expected(ref, data)
            assert (x["ret"], x["key_off"], x["key_len"]) == (rec[0], rec[1], 24) and x["accept"] == bytes(expect[:28]), i
            assert verify_header(header, x["resp"], bytes(expect), proto, 0)[0] == len(x["resp"])


# ------------------------------------------------------------------ verify

def test_directed_table(header):
    seen = set()
    for name, data, offered, max_head in CC.directed_table():
        want = CO.verify(data, CC.EXPECT, offered, max_head)
        assert verify_header(header, data, CC.EXPECT, offered, max_head) == want, name
        assert verify_export(data, CC.EXPECT, offered, max_head) == want, name
        seen.add(CO.result_class(want))
    assert seen == set(CC.CLASSES)
    by = {n: CO.verify(d, CC.EXPECT, o, m) for n, d, o, m in CC.directed_table()}
    assert [by["status %d" % c][2] for c in (200, 302, 401)] == [200, 302, 401] and by["status line malformed"][2] == 0
    assert by["HTTP/1.0"][:3] == (-1, CO.STATUS, 101) and by["101 with no reason phrase"][0] > 0
    assert by["protocol in the middle of the offered"][4] == 2 and by["a bare LF LF"][0] == 0
    assert by["max_head one below T + 4"][1] == CO.TOO_LONG and by["max_head at T + 4"][0] == by["max_head one above T + 4"][0] > 0


def test_header_matches_the_model_on_the_seeded_sweep(header, sweep):
    cases, exps = sweep
    for i, ((d, off, mh), x) in enumerate(zip(cases, exps)):
        assert verify_header(header, d, CC.EXPECT, off, mh) == x, i


def test_exported_host_entry_matches_the_seeded_sweep(sweep):
    cases, exps = sweep
    for i, ((d, off, mh), x) in enumerate(zip(cases[::4], exps[::4])):
        assert verify_export(d, CC.EXPECT, off, mh) == x, 4 * i


def test_seeded_sweep_covers_every_class(sweep):
    """each class of result (ok, ok with protocol, incomplete and the seven reasons) is at least 5 %
    of the seeded responses, on the model's own results: a degenerate generator cannot pass quietly"""
    cases, exps = sweep
    assert len(cases) == 4096
    n = float(len(cases))
    cov = {c: sum(CO.result_class(x) == c for x in exps) / n for c in CC.CLASSES}
    assert len(cov) == 10 and all(v >= 0.05 for v in cov.values()), cov
    assert {len(d) // 1024 for d, _o, _m in cases} >= {0, 1, 2}          # one, two and three rounds of the kernel


def test_expect_differs_per_nonce(header):
    """a response made for another nonce fails ACCEPT; for its own it passes"""
    a, b = CO.expect_of(nonce_of(1)), CO.expect_of(nonce_of(2))
    r = CC.good(acc=a[:28])
    assert verify_header(header, r, a, b"", 0)[0] == len(r)
    assert verify_header(header, r, b, b"", 0)[:2] == (-1, CO.ACCEPT)


def test_round_edge_inputs_exist():
    """the generators of tests/test_gpu_client.py really place a line start in the last lane of a
    round (1008..1023) and in the first lane of the next, for every header name, the 28 accept bytes
    astride the round edge, and the terminator at every offset 1000..1060"""
    for which in range(5):
        starts = {CC.header_at(which, off).index(CC.NAMES[which] + b":") for off in range(1000, 1051)}
        assert any(1008 <= p < 1024 for p in starts) and any(1024 <= p < 1040 for p in starts), which
        assert 1023 in starts and 1024 in starts
    d = CC.header_at(2, 1000, b" ")
    a = d.index(CC.ACC)
    assert a < 1024 < a + 28                                    # the 28 accept bytes cross the round edge
    t = [CC.terminator_at(o) for o in range(1000, 1061)]
    assert {x.index(b"\r\n\r\n") for x in t} == set(range(1000, 1061))
    assert {1007, 1023, 1039} <= {x.index(b"\r\n\r\n") for x in t}   # "\r\n" split over chunk edges and the round edge
    cases = CC.header_cases()
    assert len(cases) == 5 * 51 + 131 and all(CO.verify(d, CC.EXPECT, o)[0] > 0 for d, o in cases)


# ------------------------------------------------------------------ arguments, constants, symbols

def test_exported_host_entries_refuse_bad_arguments():
    lib = _lib.load_cli_lib()
    cv = np.full(1, 7, np.uint32).repeat(8)
    buf, ex = np.zeros(64, np.uint8), np.zeros(32, np.uint8)
    for flags in (1, 2, 0x80000000):
        assert lib.websocketframeClientVerifyHost(buf.ctypes.data, 10, flags, ex.ctypes.data, None, 0, 0, cv.ctypes.data) < 0
        assert (cv == 7).all() and lib.websocketframeGpuLastError() != b""
        rd = np.full(4, 7, np.uint32)
        assert lib.websocketframeClientRequestHost(buf.ctypes.data, 1, None, 0, None, 0, ex.ctypes.data, flags, None, 0,
                                                   ex.ctypes.data, rd.ctypes.data) < 0
        assert (rd == 7).all()
    assert lib.websocketframeClientVerifyHost(buf.ctypes.data, 10, 0, ex.ctypes.data, None, 0, 0, None) < 0
    assert lib.websocketframeClientVerifyHost(buf.ctypes.data, 10, 0, None, None, 0, 0, cv.ctypes.data) < 0
    assert lib.websocketframeClientRequestHost(buf.ctypes.data, 1, None, 0, None, 0, ex.ctypes.data, 0, None, 0, ex.ctypes.data,
                                               None) < 0
    assert lib.websocketframeClientRequestHost(buf.ctypes.data, 1, None, 0, None, 0, None, 0, None, 0, ex.ctypes.data,
                                               cv.ctypes.data) < 0
    assert (cv == 7).all()
    # a length the int return cannot express: flagged, never read
    assert lib.websocketframeClientVerifyHost(buf.ctypes.data, 1 << 31, 0, ex.ctypes.data, None, 0, 0, cv.ctypes.data) == 0
    assert tuple(int(v) for v in cv.view(W.CLI_VERIFY_DTYPE)[0]) == (-1, 0, 0, W.CLI_NONE, 0, W.CLI_NONE, W.CLI_ERR_SEG_LEN, 0)
    assert CO.verify(b"", CC.EXPECT)[0] == 0


def test_cli_library_exports():
    """libwsframe_amd_cli.so's symbol table is libwsframe_amd_send.so's plus exactly the four names
    wsframe_amd_client.h marks; every older library exports none of them"""
    src = open(HEADER).read()
    marked = set(re.findall(r"WSFRAME_AMD_CLI_EXPORT[^;]*?\b(websocketframe\w+)\s*\(", src, re.S))
    assert marked == set(_lib.CLI_EXPORTS) and len(marked) == 4
    assert os.path.exists(_lib.CLI_LIB_PATH), "libwsframe_amd_cli.so is not built"
    assert dynamic_symbols(_lib.CLI_LIB_PATH) == dynamic_symbols(_lib.SEND_LIB_PATH) | marked
    for path in (_lib.LIB_PATH, _lib.CTL_LIB_PATH, _lib.TEXT_LIB_PATH, _lib.PROTO_LIB_PATH, _lib.HS_LIB_PATH,
                 _lib.REPLY_LIB_PATH, _lib.SEND_LIB_PATH, _lib.BENCH_LIB_PATH):
        assert not dynamic_symbols(path) & marked, path


def test_constants_agree():
    src = open(HEADER).read()
    consts = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define WEBSOCKET_CLI_(\w+)\s+(\w+)", src)}
    assert consts == {"NONE": W.CLI_NONE, "REQ_WRITTEN": W.CLI_REQ_WRITTEN, "REQ_NO_SPACE": W.CLI_REQ_NO_SPACE,
                      "ERR_RANGE": W.CLI_ERR_RANGE, "ERR_BYTES": W.CLI_ERR_BYTES, "ERR_SEG_LEN": W.CLI_ERR_SEG_LEN}
    assert (CO.NONE, CO.REQ_WRITTEN, CO.REQ_NO_SPACE, CO.ERR_RANGE, CO.ERR_BYTES, CO.ERR_SEG_LEN, CO.PAD) == (
        W.CLI_NONE, W.CLI_REQ_WRITTEN, W.CLI_REQ_NO_SPACE, W.CLI_ERR_RANGE, W.CLI_ERR_BYTES, W.CLI_ERR_SEG_LEN, W.BATCH_PAD)
    enum = dict((k, int(v)) for k, v in re.findall(r"WEBSOCKET_CLI_(OK|REASON_\w+) = (\d+)", src))
    assert enum == {"OK": W.CLI_OK, "REASON_STATUS": W.CLI_REASON_STATUS, "REASON_UPGRADE": W.CLI_REASON_UPGRADE,
                    "REASON_CONNECTION": W.CLI_REASON_CONNECTION, "REASON_ACCEPT": W.CLI_REASON_ACCEPT,
                    "REASON_EXTENSION": W.CLI_REASON_EXTENSION, "REASON_PROTOCOL": W.CLI_REASON_PROTOCOL,
                    "REASON_TOO_LONG": W.CLI_REASON_TOO_LONG}
    assert (CO.OK, CO.STATUS, CO.UPGRADE, CO.CONNECTION, CO.ACCEPT, CO.EXTENSION, CO.PROTOCOL, CO.TOO_LONG) == tuple(range(8))
    for struct, dtype in (("WebsocketClientEntry_t", W.CLI_ENTRY_DTYPE), ("WebsocketClientReqDesc_t", W.CLI_REQ_DTYPE),
                          ("WebsocketClientVerifyDesc_t", W.CLI_VERIFY_DTYPE)):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        names = re.findall(r"^\s*(?:unsigned long long|unsigned int|int) (\w+)(?:\[\d+\])?;", fields, re.M)
        assert tuple(names) == dtype.names, struct
    assert W.CLI_ENTRY_DTYPE.itemsize % 16 == 0


def test_sanitizer_program_on_the_directed_table(tmp_path):
    """the same source as a program of its own under AddressSanitizer and UBSan, run with no
    preload: every directed response from a heap buffer of exactly len + 32 bytes, and requests into
    buffers of exactly req_len bytes and of one byte less"""
    exe = str(tmp_path / "client_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DCLIENT_HOST_MAIN", SRC, "-o", exe],
                   check=True)
    path = str(tmp_path / "cases.txt")

    def hx(b):
        return b.hex() if b else "-"
    n = 0
    with open(path, "w") as f:
        for _name, data, offered, max_head in CC.directed_table():
            x = CO.verify(data, CC.EXPECT, offered, max_head)
            f.write("V %s %s %d %d %d %d %d %d %d %s\n" % (hx(data), hx(offered), max_head, x[0], x[1], x[2], x[3], x[4], x[5],
                                                           hx(CC.EXPECT)))
            n += 1
        for i in range(1, 40):
            nonce, p = nonce_of(i), b"/" + HC.filler(i * 3, i)
            proto, host = (b"", b"chat")[i % 2], (b"", b"example.com")[i % 3 == 0]
            rec, text, expect = CO.request_record(p, nonce, proto, host, 1 << 20)
            f.write("R %s %s %s %s %s %s %d\n" % (hx(p), hx(proto), hx(host), hx(nonce), hx(text), hx(expect), rec[1]))
            n += 1
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "client_host ok %d" % n, out.stdout + out.stderr
