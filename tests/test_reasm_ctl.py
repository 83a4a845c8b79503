"""WEBSOCKET_REASM_CONTROL_DIRECT without a GPU: the rule's checker (tests/reasm_ctl_oracle.py)
against the reference reactor's deliveries under a control-direct glue
(tests/golden/reassemble_ctl.json), against the plain checker where no control frame occurs,
and the library's host glue (websocketframeOnDecodeControl / -BatchControl)."""
import ctypes as C

import numpy as np
import pytest

import reasm_cases as R0
import reasm_ctl_cases as R
import util_amd
from oracle_lib import oracle_reassemble, oracle_segments
from reasm_ctl_oracle import oracle_reassemble_ctl, reactor_view_ctl
from test_abi import _Cursor, _reactor_loop, dynamic_symbols, header_symbols
from util_amd import _lib


def _cases(golden):
    cases = golden("reassemble_ctl.json")
    assert [c["name"] for c in cases] == list(R.CASES)
    for c in cases:
        wire, limit = R.build(c["name"])
        assert R.sha256(wire) == c["wire_sha256"] and len(wire) == c["wire_len"], c["name"]  # stream pinned
        assert limit == c["readcache_max"]
        yield c, wire


def _fixture_view(c):
    return (c["msg_lens"], c["bodies_sha256"], c["consumed"], c["frames"], c["detach_error"], c["pending"], c["cached"])


def _digest(v):
    return (v[0], R.sha256(v[1])) + tuple(v[2:])


def test_ctl_library_exports():
    """libwsframe_amd_ctl.so exports libwsframe_amd.so's C ABI plus exactly the entry points the
    headers mark WSFRAME_AMD_CTL_EXPORT; libwsframe_amd.so exports none of them"""
    import os
    import re
    ctl = set()
    for n in ("wsframe_amd.h", "wsframe_amd_channel.h"):
        src = open(os.path.join(_lib.REPO, "include", n)).read()
        ctl |= set(re.findall(r"WSFRAME_AMD_CTL_EXPORT[^;]*?\b(websocketframe\w+)\s*\(", src, re.S))
    assert ctl == set(_lib.CTL_EXPORTS) and len(ctl) == 3
    assert dynamic_symbols(_lib.CTL_LIB_PATH) == set(header_symbols()) | ctl
    assert not dynamic_symbols(_lib.LIB_PATH) & ctl
    lib = _lib.load_ctl_lib()
    for s in ctl:
        assert getattr(lib, s) is not None


def test_ctl_oracle_reproduces_the_fixture(golden):
    """every stream as one rx segment: the checker's complete messages in descriptor order are the
    reference reactor's deliveries, with its consumed bytes and frames, detach and cache state"""
    n = 0
    for c, wire in _cases(golden):
        _, res, msgs, regions, op, cached = oracle_reassemble_ctl(wire, [0], [len(wire)], c["frames"] + 2,
                                                                  readcache_max=c["readcache_max"])
        assert _digest(reactor_view_ctl(msgs, regions, res, op, cached, [len(wire)])) == _fixture_view(c), c["name"]
        n += 1
    assert n == 11


def test_ctl_oracle_delivery_rule_by_hand():
    """[A data][ping][B data FIN][pong][C data] -> ping, A+B (frames 0 and 2, 2 data frames), pong,
    then C pending; bodies: data upward, control downward from the region's end"""
    def frame(b0, body, key=b"\x01\x02\x03\x04"):
        return bytes([b0, 0x80 | len(body)]) + key + bytes(x ^ key[i % 4] for i, x in enumerate(body))
    wire = (frame(0x02, b"alpha") + frame(0x89, b"PING") + frame(0x80, b"beta") + frame(0x0A, b"po") +
            frame(0x00, b"gamma"))
    w = np.frombuffer(wire, dtype=np.uint8)
    n = len(wire)
    _, res, msgs, regions, op, _ = oracle_reassemble_ctl(w, [0], [n], 8)
    assert int(res[0]["n_frames"]) == 5 and int(res[0]["consumed"]) == n
    assert msgs[0] == [(n - 4, 4, 1, 1, 1, 0), (0, 9, 0, 2, 1, 0), (n - 6, 2, 3, 1, 1, 0), (9, 5, 4, 1, 0, 0)]
    assert bytes(regions[0][1]) == b"alphabetagamma" and bytes(regions[0][2]) == b"poPING" and op[0] == 1


@pytest.mark.parametrize("case", ["cfg5_shape", "open_end", "overflow_count", "boundary", "zero_len"])
def test_ctl_oracle_equals_plain_oracle_without_control_frames(case):
    wire, limit = R0.build(case)
    if case == "cfg5_shape":
        wire = wire[:4 * 16 * (1024 + 8)]
    for mf in (5, 4096):
        so, sl = [0, 0], [len(wire), len(wire)]                       # the stream with and without a message carried in
        a = oracle_reassemble(wire, so, sl, mf, [0, 1], None, limit, [0, 77])
        b = oracle_reassemble_ctl(wire, so, sl, mf, [0, 1], None, limit, [0, 77])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        for (oa, body), (ob, data, ctl) in zip(a[3], b[3]):
            assert oa == ob and np.array_equal(body, data) and len(ctl) == 0
        assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])


def test_reference_reactor_with_amd_control_glue(golden):
    """dev container only: the reference's reactor + stream hook with NetChannelExProc_t.on_decode =
    libwsframe_amd_ctl.so's websocketframeOnDecodeControl delivers the fixture's deliveries"""
    import ref_reactor as X
    if not X.available():
        pytest.skip("reference build not present (GPU box): tests/golden/reassemble_ctl.json carries the pin")
    glue = C.cast(_lib.load_ctl_lib().websocketframeOnDecodeControl, C.c_void_p).value
    for c, wire in _cases(golden):
        r = X.reactor_deliver(wire, 1500, c["readcache_max"], on_decode=glue)
        v = (r["lens"], R.sha256(r["bodies"]), r["consumed"], r["frames"], r["detach_error"], r["pending"], r["cached"])
        assert v == _fixture_view(c), c["name"]


@pytest.mark.parametrize("case", ["ping_between", "control_no_fin", "opcodes", "tail"])
def test_control_glue_batch_replay(case):
    """websocketframeOnDecodeBatchControl replays a batch decode's descriptors to the reactor loop
    exactly as websocketframeOnDecodeControl's per-frame decode drives it (pktype 0 for control
    frames, from the descriptor's type), also past a short descriptor capacity (MAX_FRAMES)"""
    lib, plain_lib = _lib.load_ctl_lib(), util_amd.load_lib()
    wire, _ = R.build(case)
    single = wire.copy()
    ref, ref_off = _reactor_loop(single, lambda p, n, r: lib.websocketframeOnDecodeControl(None, p, n, r))
    assert {t[3] for t in ref if t != "err"} == {b"\x00", b"\x06"}          # both packet types occur
    for cap in (1 << 16, 3):
        batch = wire.copy()
        od, orr = oracle_segments(batch, [0], [len(batch)], cap)  # the batch decode, in place
        desc = np.ascontiguousarray(od[:int(orr[0]["n_frames"])])
        cur = _Cursor(desc.ctypes.data, int(orr[0]["consumed"]), int(orr[0]["n_frames"]), int(orr[0]["status"]), 0,
                      batch.ctypes.data, 0)
        got, got_off = _reactor_loop(batch, lambda p, n, r: lib.websocketframeOnDecodeBatchControl(C.byref(cur), p, n, r))
        assert got == ref and got_off == ref_off, cap
        assert np.array_equal(batch[:ref_off], single[:ref_off])
    # the plain glue reports every frame as a fragment
    plain, _ = _reactor_loop(wire.copy(), lambda p, n, r: plain_lib.websocketframeOnDecode(None, p, n, r))
    assert {t[3] for t in plain if t != "err"} == {b"\x06"}
