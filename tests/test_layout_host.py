"""The two workspace layouts of util_amd/csrc/ws_layout.h — the piece workspace (batch form and the raw
stream's form) and the scratch of the raw stream's chunk-parallel walk — compiled for the host behind a
thin C shim (tests/c/layout_host.cpp). The expected offsets are written out here, independently, from the
formulas the launchers held before the header took them over; alignment, disjointness and "the views fit
inside what the caller allocates" are checked on the header's own output. CPU only: g++, ctypes, numpy."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
KIB = 1 << 10
U = np.uint64


@pytest.fixture(scope="module")
def lay(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("layout") / "liblayout_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "c", "layout_host.cpp"),
                    "-o", so_path], check=True)
    lib = C.CDLL(so_path)
    u64, vp = C.c_ulonglong, C.c_void_p
    for name, args in (("ws_layout_piece", [u64, vp, vp]), ("ws_layout_piece_bytes", [u64, vp, vp]),
                       ("ws_layout_stream", [u64, vp, vp]), ("ws_layout_carve", [u64, u64, u64, u64, u64, vp]),
                       ("ws_layout_device", [u64, u64, u64, vp]), ("ws_layout_consts", [vp])):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = args
    return lib


@pytest.fixture(scope="module")
def consts(lay):
    o = np.zeros(12, dtype=U)
    lay.ws_layout_consts(o.ctypes.data)
    names = ("shift", "D", "slots", "slast", "rec", "own", "row", "cmin", "cap_chunks", "hmax", "cap_stgn", "rw_min")
    return dict(zip(names, (int(v) for v in o)))


def test_constants(consts):
    assert consts == dict(shift=14, D=4, slots=48, slast=4096, rec=16, own=32, row=64, cmin=64 * KIB, cap_chunks=32768,
                          hmax=128 * KIB, cap_stgn=1024, rw_min=512 * KIB)


def rows(lib_fn, inp, width):
    a = np.ascontiguousarray(np.array(inp, dtype=U))
    o = np.zeros((len(a), width), dtype=U)
    lib_fn(len(a), a.ctypes.data, o.ctypes.data)
    return a, o


def up(x, a):
    return (x + U(a - 1)) & ~U(a - 1)


SPANS = sorted(k * 16 * KIB + d for k in (0, 1, 2, 3, 1024) for d in (-16, -15, -1, 0, 1, 15, 16) if k * 16 * KIB + d >= 0)
LEADS = range(16)
LOS = (0, 1, 16383, 16384)
NSEGS = (1, 2, 7, 8, 9, 1 << 20)
MAXFS = (1, 16, 65536)


def piece_bytes(span, nseg, maxf):
    """ws_piece_workspace_bytes as it stood in ws_piece.hip"""
    npieces = (span + U(15)) // U(16384) + U(2)
    b = (U(16) + npieces * U(8) + U(15)) & ~U(15)
    b = (b + nseg * U(4) + U(31)) & ~U(31)
    b = b + nseg * U(16)
    return b + nseg * maxf * U(16) + U(16)


def test_piece_batch_form(lay):
    """piece_scan_args' views as they stood, for every span, base phase, range start, nseg and max_frames"""
    inp = [(lo + lead, lo + lead + span, nseg, maxf, 1)
           for span, lead, lo, nseg, maxf in itertools.product(SPANS, LEADS, LOS, NSEGS, MAXFS)]
    a, o = rows(lay.ws_layout_piece, inp, 11)
    lo, hi, nseg, maxf = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    npieces, pbase, c_lo, c_hi, disorder, nonuni, ptr, nwork, segr, items, end = o.T
    want_np = np.where(hi > lo, ((np.maximum(hi, U(1)) - U(1)) >> U(14)) - (lo >> U(14)) + U(1), U(0))
    assert (npieces == want_np).all()
    assert (pbase == lo >> U(14)).all() and (c_lo == lo >> U(4)).all() and (c_hi == (hi + U(15)) >> U(4)).all()
    assert (disorder == 0).all() and (nonuni == 4).all() and (ptr == 16).all()
    b = (U(16) + want_np * U(8) + U(15)) & ~U(15)
    assert (nwork == b).all()
    b = (b + nseg * U(4) + U(31)) & ~U(31)
    assert (segr == b).all()
    b = b + nseg * U(16)
    assert (items == b).all() and (end == b + nseg * maxf * U(16)).all()
    # on the header's own output: alignment, no overlap, and the end inside what the caller allocates
    for r in (ptr, nwork, items):
        assert (r % U(16) == 0).all()
    assert (segr % U(32) == 0).all()
    assert (ptr + npieces * U(8) <= nwork).all() and (nwork + nseg * U(4) <= segr).all()
    assert (segr + nseg * U(16) <= items).all()
    span = hi - lo
    _, got_bytes = rows(lay.ws_layout_piece_bytes, np.stack([span, nseg, maxf], axis=1), 1)
    got_bytes = got_bytes[:, 0]
    assert (got_bytes == piece_bytes(span, nseg, maxf)).all()
    assert (end <= got_bytes).all()
    # ... also when the segments' range is shorter than the span the caller sized the workspace for
    for less in (1, 15, 16, 16383):
        keep = span >= U(less)
        a2 = a[keep].copy()
        a2[:, 1] -= U(less)
        _, o2 = rows(lay.ws_layout_piece, a2, 11)
        assert (o2[:, 10] <= got_bytes[keep]).all()


def test_piece_stream_form(lay):
    """the raw-stream entry's views and its segment pair as they stood"""
    inp = [(lead, length, maxf) for lead, length, maxf in itertools.product(LEADS, [0] + SPANS, MAXFS)]
    a, o = rows(lay.ws_layout_stream, inp, 13)
    lead, length, maxf = a.T
    npieces, pbase, c_lo, c_hi, disorder, nonuni, ptr, nwork, segr, items, end, seg, nbytes = o.T
    tot = length + lead
    want_np = np.where(tot > 0, ((np.maximum(tot, U(1)) - U(1)) >> U(14)) + U(1), U(0))
    assert (npieces == want_np).all()
    assert (pbase == 0).all() and (c_lo == 0).all() and (c_hi == (tot + U(15)) >> U(4)).all()
    assert (disorder == 0).all() and (nonuni == 4).all() and (ptr == 16).all() and (segr == 0).all()
    b = (U(16) + want_np * U(8) + U(15)) & ~U(15)
    assert (nwork == b).all()
    b = (b + U(4) + U(15)) & ~U(15)
    assert (items == b).all() and (end == b + maxf * U(16)).all()
    pws = piece_bytes(length, U(1), maxf)
    assert (seg == (pws + U(15)) & ~U(15)).all() and (nbytes == pws + U(64)).all()
    for r in (ptr, nwork, items, seg):
        assert (r % U(16) == 0).all()
    assert (ptr + npieces * U(8) <= nwork).all() and (nwork + U(4) <= items).all()
    assert (end <= seg).all()                       # the items end before the segment pair ...
    assert (seg + U(16) <= nbytes).all()            # ... which lies inside what the entry allocates
    # one function counts the pieces: the stream's own expression is the batch count from origin 0, and from
    # the base phase too whenever the stream holds a byte
    _, ob = rows(lay.ws_layout_piece, np.stack([lead, tot, U(1) + U(0) * lead, maxf, U(0) * lead], axis=1), 11)
    assert (ob[length > 0, 0] == npieces[length > 0]).all()


def walk_want(c, chunks, stg_words, cand_words, plan_bytes, link_bytes):
    """the chunk-walk scratch as rw_dev_layout carved it (plan_bytes > 0), and the same order for the
    host-linked walk (plan_bytes 0: a 256-B report head, one row per chunk, no link table)"""
    u = lambda x: (x + 255) & ~255
    sizes = [("plan", u(plan_bytes) if plan_bytes else 256), ("nrec", u(chunks * 16)), ("dx", u(chunks * c["D"] * 8)),
             ("recs", u((chunks * c["slots"] + c["slast"]) * c["rec"])), ("own", u(chunks * c["D"] * c["own"])),
             ("tab", u((chunks + (2 if plan_bytes else 0)) * c["row"])), ("stg", u(stg_words * 4)), ("cand", u(cand_words * 8)),
             ("lk", u(chunks * link_bytes))]
    off, o = {}, 0
    for name, sz in sizes:
        off[name] = o
        o += sz
    return off, dict(sizes), o


def check_walk(c, got, chunks, stg_words, cand_words, plan_bytes, link_bytes):
    names = ("plan", "nrec", "dx", "recs", "own", "tab", "stg", "cand", "lk")
    off, size, total = walk_want(c, chunks, stg_words, cand_words, plan_bytes, link_bytes)
    g = dict(zip(names, got[:9]))
    assert g == off, (chunks, g, off)
    assert got[9] == total
    # 256-B aligned and disjoint, each region holding its entries
    need = dict(plan=plan_bytes or 256, nrec=chunks * 16, dx=chunks * c["D"] * 8,
                recs=(chunks * c["slots"] + c["slast"]) * c["rec"], own=chunks * c["D"] * c["own"],
                tab=(chunks + (2 if plan_bytes else 0)) * c["row"], stg=stg_words * 4, cand=cand_words * 8, lk=chunks * link_bytes)
    ends = [g[n] for n in names[1:]] + [got[9]]
    for n, e in zip(names, ends):
        assert g[n] % 256 == 0 and g[n] + need[n] <= e, (n, chunks)
    # the zeroed range is exactly nrec + dx; the copied-back range is one piece: nrec, dx, recs, own
    assert g["nrec"] + got[10] == g["recs"] and g["dx"] == g["nrec"] + size["nrec"] and g["recs"] == g["dx"] + size["dx"]
    assert g["nrec"] + got[11] == g["tab"] and g["own"] == g["recs"] + size["recs"] and g["tab"] == g["own"] + size["own"]


def walk_lengths(c):
    out = [c["rw_min"], c["rw_min"] + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 40]
    cmin = c["cmin"]
    while (c["cap_chunks"] - 2) * cmin <= 1 << 40:                  # ceil(len / cmin) + 2 == the cap, and one byte more
        out += [(c["cap_chunks"] - 2) * cmin - 1, (c["cap_chunks"] - 2) * cmin, (c["cap_chunks"] - 2) * cmin + 1]
        cmin <<= 1
    return out


def test_chunk_walk_device_layout(lay, consts):
    c = consts
    doubled = set()
    for length, (plan_bytes, link_bytes) in itertools.product(walk_lengths(c), ((336, 32), (1, 32), (256, 8), (257, 32))):
        o = np.zeros(16, dtype=U)
        lay.ws_layout_device(length, plan_bytes, link_bytes, o.ctypes.data)
        got = [int(v) for v in o]
        cmin = c["cmin"]
        while (length + cmin - 1) // cmin + 2 > c["cap_chunks"]:
            cmin <<= 1
        nch = (length + cmin - 1) // cmin + 2
        cand = min(nch * (c["hmax"] // 32), length // 1024 + 65536)
        stg = min(nch * c["D"] * c["cap_stgn"], length // 256 + 65536)
        assert got[:4] == [cmin, nch, cand, stg], length
        assert nch <= c["cap_chunks"]
        doubled.add(cmin)
        check_walk(c, got[4:], nch, stg, cand, plan_bytes, link_bytes)
    assert len(doubled) >= 10 and c["cmin"] in doubled


def test_chunk_walk_host_layout(lay, consts):
    c = consts
    for chunks, stgn, capc in itertools.product((1, 2, 15, 16, 17, 1000, 32768, 1 << 24), (256, 4096), (128, 4096)):
        o = np.zeros(12, dtype=U)
        lay.ws_layout_carve(chunks, chunks * c["D"] * stgn, chunks * capc, 0, 0, o.ctypes.data)
        got = [int(v) for v in o]
        check_walk(c, got, chunks, chunks * c["D"] * stgn, chunks * capc, 0, 0)
        assert got[0] == 0 and got[1] == 256 and got[8] == got[9]    # the report head; no link table
