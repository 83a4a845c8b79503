"""The chunk-chain link rule the raw stream's linkers share (util_amd/csrc/ws_link.h: the record
pools, the lookups and rw_link_decide), compiled for the host inside a scalar model of the whole
chunk-parallel walk (tests/c/link_host.cpp) and held against the oracle: frame offsets, consumed,
n_frames and status over [0, len). The model's geometry is free, so 4 KiB chunks with 512 B windows
reach every branch on streams of 64-256 KiB; each case also asserts, through the model's counters,
that it took the branch it is named for. CPU only: g++, ctypes and numpy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle_lib import oracle_segments
from util_amd.wsframe import SEGRES_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
CH, WIN = 4096, 512                       # chunk and window bytes
COUNTERS = ["rows_group", "rows_owner", "chunk_walks", "clipped", "over", "pool_s1", "pool_slast", "dead",
            "skipped", "max_prefix", "max_rest", "no_window"]
WALK, GROUP, OWNER = 0, 1, 2              # RW_LINK_*
SEG_OK, SEG_MAX_FRAMES = 0, 1


@pytest.fixture(scope="module")
def link(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("link") / "liblink_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "c", "link_host.cpp"),
                    "-o", so_path], check=True)
    lib = C.CDLL(so_path)
    lib.ws_link_host_stream.restype = C.c_int
    lib.ws_link_host_stream.argtypes = [C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_uint,
                                        C.c_ulonglong, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_uint]
    return lib.ws_link_host_stream


def frame(rng, plen, masked=True, b0=0x82):
    m = 0x80 if masked else 0
    if plen < 126:
        h = bytes([b0, m | plen])
    elif plen <= 0xFFFF:
        h = bytes([b0, m | 126]) + plen.to_bytes(2, "big")
    else:
        h = bytes([b0, m | 127]) + plen.to_bytes(8, "big")
    return h + rng.integers(0, 256, (4 if masked else 0) + plen, dtype=np.uint8).tobytes()


def frames(rng, nbytes, lo=0, hi=300):
    """masked client frames of lo..hi payload bytes, back to back, until nbytes"""
    parts, total = [], 0
    while total < nbytes:
        parts.append(frame(rng, int(rng.integers(lo, hi + 1)), b0=int(rng.choice([0x01, 0x02, 0x80, 0x81, 0x82, 0x89]))))
        total += len(parts[-1])
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy()


def frame_offs(wire, mf=1 << 16):
    od, orr = oracle_segments(wire.copy(), [0], [len(wire)], mf)
    return od["frame_off"][:int(orr[0]["n_frames"])]


def start_at(wire, at):
    """the first frame start at or after byte `at`"""
    fo = frame_offs(wire)
    return int(fo[np.searchsorted(fo, at)])


def splice(wire, at, ins):
    """`ins` put in front of the first frame that starts at or after `at`"""
    f = start_at(wire, at)
    return np.concatenate([wire[:f], np.frombuffer(ins, dtype=np.uint8), wire[f:]]), f


def hdr64(plen, masked=True):
    return bytes([0x82, 0xFF if masked else 0x7F]) + int(plen).to_bytes(8, "big") + (b"\x11\x22\x33\x44" if masked else b"")


def run_model(link, wire, P, nf, max_frames, stgn):
    buf = np.zeros(len(wire) + 64, dtype=np.uint8)
    buf[:len(wire)] = wire
    offs = np.full(max_frames, 2 ** 64 - 1, dtype=np.uint64)
    res = np.zeros(1, dtype=SEGRES_DTYPE)
    cnt = np.zeros(len(COUNTERS), dtype=np.uint64)
    trace = np.zeros(2 * 1024, dtype=np.uint32)
    steps = link(buf.ctypes.data, len(buf), len(wire), P, nf, CH, WIN, stgn, max_frames, 1, offs.ctypes.data,
                 res.ctypes.data, cnt.ctypes.data, trace.ctypes.data, 1024)
    assert 0 <= steps <= 1024, "the model gave up: %d" % steps
    od, orr = oracle_segments(wire.copy(), [0], [len(wire)], max_frames)
    n = int(orr[0]["n_frames"])
    assert tuple(res[0]) == tuple(orr[0]), (tuple(res[0]), tuple(orr[0]))
    assert nf <= n and np.array_equal(offs[nf:n], od["frame_off"][nf:n]), "frame offsets"
    k = dict(zip(COUNTERS, (int(x) for x in cnt)))
    k["steps"] = steps
    return k, trace[:2 * steps].reshape(-1, 2), orr[0]


def both(link, wire, max_frames=1 << 15, stgn=64):
    """the walk from P = 0 and, behind nine more frames (1,003 bytes: another 16-B phase), from a P
    inside the stream with nf = 9: the same chunk grid over the same bytes both times; yields the
    counters, the chain's (chunk, kind) steps, the oracle's result and the bytes put in front"""
    yield run_model(link, wire, 0, 0, max_frames, stgn) + (0,)
    rng = np.random.default_rng(5)
    pre = b"".join(frame(rng, n) for n in (100, 0, 125, 126, 7, 300, 60, 131, 94))
    assert len(pre) == 1003
    wire = np.concatenate([np.frombuffer(pre, dtype=np.uint8), wire])
    yield run_model(link, wire, len(pre), 9, max_frames + 9, stgn) + (len(pre),)


def test_every_chunk_linked_from_records(link):
    """client frames of 0-300 B, all masked: one owner row per chunk, no chunk walk"""
    wire = frames(np.random.default_rng(1), 128 << 10)
    for k, trace, r, sh in both(link, wire):
        assert int(r["consumed"]) == len(wire) + sh and int(r["status"]) == SEG_OK
        assert k["chunk_walks"] == 0 and k["rows_group"] == 0 and k["rows_owner"] == k["steps"] >= 32
        assert (trace[:, 0] == np.arange(k["steps"])).all()


def test_frame_longer_than_the_window_at_a_chunk_start(link):
    """a 1000 B frame over the first bytes of chunk 5: no record at the entry, a chunk walk, then records"""
    rng = np.random.default_rng(2)
    wire = frames(rng, 64 << 10)
    f = int(frame_offs(wire)[np.searchsorted(frame_offs(wire), 5 * CH) - 1])      # the last start before chunk 5
    wire = np.concatenate([wire[:f], np.frombuffer(frame(rng, 1000), dtype=np.uint8), wire[f:]])
    for k, trace, r, sh in both(link, wire):
        assert int(r["consumed"]) == len(wire) + sh
        assert k["no_window"] >= 1 and k["chunk_walks"] >= 1
        walked = np.nonzero(trace[:, 1] == WALK)[0]
        assert trace[walked[0], 0] == 5 and (trace[walked[-1] + 1:, 1] == OWNER).all() and walked[-1] + 1 < len(trace)


def test_frame_longer_than_a_chunk(link):
    """a frame of two chunks and a bit: the chain skips a chunk"""
    rng = np.random.default_rng(3)
    wire, f = splice(frames(rng, 64 << 10), 5 * CH + 1000, frame(rng, 2 * CH + 100))
    for k, trace, r, sh in both(link, wire):
        assert int(r["consumed"]) == len(wire) + sh
        assert k["skipped"] >= 1 and 6 not in trace[:, 0] and 5 in trace[:, 0]


def test_stream_ends_in_a_middle_chunks_window(link):
    """an incomplete frame (a 1 MiB length, three chunks of bytes after it) at chunk 5's first frame
    start: a stream-ending record of a middle chunk (the RW_S1 pool)"""
    rng = np.random.default_rng(4)
    wire = frames(rng, 64 << 10)
    f = start_at(wire, 5 * CH)
    wire = np.concatenate([wire[:f], np.frombuffer(hdr64(1 << 20), dtype=np.uint8),
                           rng.integers(0, 256, 3 * CH, dtype=np.uint8)])
    for k, trace, r, sh in both(link, wire):
        assert int(r["consumed"]) == f + sh and int(r["status"]) == SEG_OK
        assert k["pool_s1"] == 1 and k["rows_group"] == 1 and k["chunk_walks"] == 0 and tuple(trace[-1]) == (5, GROUP)


def test_stream_ends_in_the_last_chunks_window(link):
    """the stream cut three bytes into the first frame of its last chunk: the RW_SLAST pool"""
    wire = frames(np.random.default_rng(6), 64 << 10)
    f = start_at(wire, 9 * CH)
    wire = wire[:f + 3].copy()
    for k, trace, r, sh in both(link, wire):
        assert int(r["status"]) == SEG_OK and int(r["n_frames"]) > 0
        assert k["pool_slast"] == 1 and k["rows_group"] == 1 and k["chunk_walks"] == 0 and tuple(trace[-1]) == (9, GROUP)


@pytest.mark.parametrize("where", ["prefix", "staged", "rest"])
def test_max_frames(link, where):
    """max_frames reached in chunk 5: inside the window prefix (a group row), inside the staged frames
    (n_par clipped) and, with 8 staged frames, in the rest of the owner walk; the three values are the
    oracle's frame counts at byte offsets inside those parts"""
    wire = frames(np.random.default_rng(7), 64 << 10)
    at, stgn = {"prefix": (5 * CH + 400, 64), "staged": (5 * CH + 2000, 64), "rest": (5 * CH + 3500, 8)}[where]
    mf = int(np.searchsorted(frame_offs(wire), at))
    for k, trace, r, sh in both(link, wire, mf, stgn):
        assert int(r["status"]) == SEG_MAX_FRAMES and trace[-1, 0] == 5
        assert (k["max_prefix"], k["clipped"], k["max_rest"]) == {"prefix": (1, 0, 0), "staged": (0, 1, 0),
                                                                  "rest": (0, 0, 1)}[where]
        assert k["chunk_walks"] == 0


def test_more_frames_than_staging(link):
    """frames of 0-20 B with 8 staged frames per owner: every row goes on at the owner's `over`"""
    wire = frames(np.random.default_rng(8), 64 << 10, 0, 20)
    for k, trace, r, sh in both(link, wire, 1 << 15, 8):
        assert int(r["consumed"]) == len(wire) + sh
        assert k["chunk_walks"] == 0 and k["over"] == k["rows_owner"] >= 16


def test_unmasked_frame_in_a_masked_stream(link):
    """one unmasked frame behind chunk 5's window: its owner walk is dead, the chunk is walked, the
    chunks after it are linked from records again"""
    rng = np.random.default_rng(9)
    wire, f = splice(frames(rng, 64 << 10), 5 * CH + 1500, frame(rng, 200, masked=False))
    for k, trace, r, sh in both(link, wire):
        assert int(r["consumed"]) == len(wire) + sh
        assert k["dead"] == 1 and k["chunk_walks"] == 1
        i = int(np.nonzero(trace[:, 1] == WALK)[0][0])
        assert trace[i, 0] == 5 and (trace[i + 1:, 1] == OWNER).all() and i + 1 < len(trace)


def test_garbage_mid_stream(link):
    """37 random bytes at a frame start: the reactor reads them as headers, and so does the walk"""
    rng = np.random.default_rng(10)
    wire, f = splice(frames(rng, 64 << 10), 5 * CH + 1500, rng.integers(0, 256, 37, dtype=np.uint8).tobytes())
    for k, trace, r, sh in both(link, wire):
        assert k["dead"] + k["chunk_walks"] + k["pool_s1"] >= 1 and 5 in trace[:, 0]


@pytest.mark.parametrize("plen,status", [((1 << 64) - 1, -2), (1 << 50, 0)])
def test_bad_64bit_length(link, plen, status):
    """a masked 64-bit length that wraps (an error status) and one with non-zero top bytes (an incomplete
    frame) behind chunk 5's window: implausible to the speculation, so the owner is dead and the
    chunk's walk ends the stream by the step rule"""
    rng = np.random.default_rng(11)
    wire, f = splice(frames(rng, 64 << 10), 5 * CH + 1500, hdr64(plen) + b"ABCDEFGH")
    for k, trace, r, sh in both(link, wire):
        assert int(r["status"]) == status and int(r["consumed"]) == f + sh
        assert k["dead"] == 1 and tuple(trace[-1]) == (5, WALK)
