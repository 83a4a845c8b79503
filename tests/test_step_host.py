"""The reactor-loop step rule the walk kernels share (util_amd/csrc/ws_step.h: ws_parse and
ws_cand_code), compiled for the host and run one candidate at a time over every directed
decode case, against the oracle. CPU only: g++, ctypes and numpy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dec_cases
from oracle_lib import oracle_segments, used_descs
from util_amd.wsframe import DESC_DTYPE, SEGRES_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = dec_cases.catalogue()


@pytest.fixture(scope="module")
def step(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("step") / "libstep_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "c", "step_host.cpp"),
                    "-o", so_path], check=True)
    lib = C.CDLL(so_path)
    lib.ws_step_host_segment.restype = None
    lib.ws_step_host_segment.argtypes = [C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_uint,
                                         C.c_void_p, C.c_void_p]
    return lib.ws_step_host_segment


def check(step, wire, seg_off, seg_len, max_frames, what):
    wire = np.ascontiguousarray(wire, dtype=np.uint8)
    nseg = len(seg_off)
    desc = np.zeros(max(1, nseg * max_frames), dtype=DESC_DTYPE)
    res = np.zeros(max(1, nseg), dtype=SEGRES_DTYPE)
    for s in range(nseg):
        step(wire.ctypes.data, len(wire), int(seg_off[s]), int(seg_len[s]), max_frames,
             desc[s * max_frames:].ctypes.data, res[s:].ctypes.data)
    od, orr = oracle_segments(wire.copy(), seg_off, seg_len, max_frames)
    res = res[:nseg]
    bad = np.nonzero(res != orr)[0]
    assert len(bad) == 0, "%s: segment %d result %s, oracle %s" % (what, bad[0], res[bad[0]], orr[bad[0]])
    assert np.array_equal(used_descs(desc, res, max_frames), used_descs(od, orr, max_frames)), what + ": descriptors"


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_step_rule_matches_oracle(step, case):
    """every catalogue case at shifts 0 and 5, every segment, every listed max_frames"""
    cid, builder, kwargs, mfs = case
    for shift in (0, 5):
        wire, so, sl, _mf = builder(lead0=shift, **kwargs)[:4]
        for mf in mfs:
            check(step, wire, so, sl, mf, "%s shift %d max_frames %d" % (cid, shift, mf))


def hdr64(plen, masked):
    return bytes([0x82, 0xFF if masked else 0x7F]) + int(plen).to_bytes(8, "big") + (b"\x11\x22\x33\x44" if masked else b"")


def test_step_rule_64bit_headers(step):
    """64-bit length headers with nothing (or a few bytes) after them: lengths past 2^31 and 2^32
    that exceed the segment come out incomplete, an unmasked length whose sum with the header
    wraps to 0 or to 5 is the reference's frame with ret 0 / ret 5, and a masked header whose
    hdr + plen wraps is WEBSOCKET_SEG_ERR_LEN_WRAP"""
    tail = b"ABCDEFGH"
    segs = [hdr64(n, m) + t for m in (False, True) for t in (b"", tail)
            for n in ((1 << 31) - 14, 1 << 31, (1 << 32) - 10, (1 << 32) + 100, 1 << 63, (1 << 64) - 15)]
    segs += [hdr64((1 << 64) - 10, False), hdr64((1 << 64) - 5, False) + tail,      # unmasked wraps: ret 0, ret 5
             hdr64((1 << 64) - 1, True) + tail, hdr64((1 << 64) - 14, True) + tail,  # masked wraps: LEN_WRAP
             dec_cases.fr(np.random.default_rng(1), 9)[0] + hdr64((1 << 64) - 3, True) + tail]
    wire, so, sl = bytearray(b"\xa5" * 3), [], []
    for sg in segs:
        so.append(len(wire))
        sl.append(len(sg))
        wire += sg + b"\xa5" * (len(sg) % 3)
    wire = np.frombuffer(bytes(wire), dtype=np.uint8)
    for mf in (1, 4):
        check(step, wire, so, sl, mf, "64-bit headers max_frames %d" % mf)
    _od, orr = oracle_segments(wire.copy(), so, sl, 4)
    assert [int(x) for x in orr["status"][-3:]] == [-2, -2, -2]
    assert int(orr["n_frames"][-1]) == 1 and all(int(x) == 0 for x in orr["n_frames"][:-1][:24])
