"""Inputs aimed at the inflate kernel's Io (util_amd/csrc/ws_inflate.hip), which no host test reaches:
the wave-wide match copy (dist against len against the 64 lanes, k % dist, the `fenced` skip), the
literal run flushed at exactly 64, the 16-byte stored copy with its head and tail, the stored block
that runs on into the virtual 00 00 FF FF tail, and the 256-byte input window with its byte-by-byte
end dwords. numpy and zlib only: tests/test_inflate_dev_cases.py holds every body against the oracle
and the host rule without a GPU, tests/test_gpu_inflate_geometry.py runs them on the device. Expected
outputs come from inflate_oracle.py, never from here."""
import functools
import struct
import zlib

import numpy as np

import inflate_cases as IC

GRID_P = (1, 2, 63, 64, 65, 66, 127, 128, 129, 300)
GRID_DIST = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 258, 259)
GRID_LEN = (3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193, 257, 258)
GRID_COUNT = 2945

RUN = 64                                  # the kernel's literal run (InfLds::lit)
STREAM_LITS = (1, 2, 62, 63, 64, 65, 66, 130)
STREAM_LENS = (3, 4, 63, 64, 65, 127, 128, 129, 257, 258)
STREAM_DISTS = (1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 1000, None)        # None: the whole output so far

STORED_N = tuple(range(41)) + (47, 48, 49, 63, 64, 65, 255, 256, 257, 1000, 1040, 65535)
STORED_PAIRS = (1, 15, 16, 17, 33, 1040)  # the sizes that must see every (source, destination) residue pair
STORED_TWO = ((1, 33), (15, 17), (16, 16), (17, 1040), (33, 15), (40, 1))
STORED_TAIL = ((4, 3), (7, 3), (6, 2), (4, 0), (5, 3), (2, 0), (5, 0))   # (LEN, body bytes behind the header)
STORED_DATA_AT = 5                        # a stored body's first data byte: the block header's byte, LEN, NLEN


def lits(rng, n):
    return [int(v) for v in rng.integers(0, 256, n, dtype=np.uint8)]


@functools.lru_cache(maxsize=None)
def match_grid():
    """[(p, dist, len, ops, body)]: p random literals, the match (len, dist), three literals and a
    match (5, len + 3) that reads back across the first, as one fixed-Huffman message"""
    rng = np.random.default_rng(2945)
    out = []
    for p in GRID_P:
        for dist in GRID_DIST:
            if dist > p:
                continue
            for ln in GRID_LEN:
                ops = lits(rng, p) + [(ln, dist)] + lits(rng, 3) + [(5, ln + 3)]
                out.append((p, dist, ln, ops, IC.fixed_block(ops)))
    return out


def stream_ops(rng, target=3000):
    """literal runs and matches drawn from the STREAM_ sets until `target` bytes stand"""
    ops, pos = [], 0
    while pos < target:
        if pos == 0 or rng.random() < 0.4:
            n = int(rng.choice(STREAM_LITS))
            ops += lits(rng, n)
            pos += n
        else:
            d = STREAM_DISTS[int(rng.integers(0, len(STREAM_DISTS)))]
            d = pos if d is None else min(d, pos)
            ln = int(rng.choice(STREAM_LENS))
            ops.append((ln, min(d, 32768)))
            pos += ln
    return ops


@functools.lru_cache(maxsize=None)
def token_streams(n=500, seed=64):
    """[(ops, body)]: n seeded fixed-block streams of about 3 KB of output"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ops = stream_ops(rng)
        out.append((ops, IC.fixed_block(ops)))
    return out


def io_trace(ops):
    """what the kernel's Io does for a token list, restated: one record per match,
    (pos, dist, len, run, fence, prev): `run` the literals flushed just before it (0: none pending),
    `fence` whether its source ends above the position the last wait covered (the wait is taken,
    else skipped), `prev` the previous match's (pos, len) or None; and the list of flushed literal
    runs [(pos, n)]"""
    pos, nlit, litpos, fenced, prev = 0, 0, 0, 0, None
    matches, runs = [], []
    for op in ops:
        if isinstance(op, int):
            if nlit == 0:
                litpos = pos
            nlit += 1
            pos += 1
            if nlit == RUN:
                runs.append((litpos, nlit))
                nlit = 0
            continue
        ln, dist = op
        if nlit:
            runs.append((litpos, nlit))
        fence = pos - dist + min(ln, dist) > fenced
        matches.append((pos, dist, ln, nlit, fence, prev))
        if fence:
            fenced = pos
        nlit, prev = 0, (pos, ln)
        pos += ln
    if nlit:
        runs.append((litpos, nlit))
    return matches, runs


def stored_block(data, final=0, length=None):
    n = len(data) if length is None else length
    return bytes([final]) + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(data)


@functools.lru_cache(maxsize=None)
def stored_grid():
    """[(name, body, n)]: level-0 bodies of STORED_N bytes (n: the size, the data at STORED_DATA_AT);
    two-block bodies, the second block's destination wherever the first ended (n None); stored blocks
    whose LEN takes its last bytes from the virtual tail (n None)"""
    rng = np.random.default_rng(16)
    out = []
    for n in STORED_N:
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        # (zlib splits 65,535 bytes in two blocks: that one is written out here, LEN FFFF in one block)
        body = IC.deflate(data, 0) if n < 65535 else stored_block(data) + b"\0"
        assert n == 0 or body[:STORED_DATA_AT] == stored_block(b"", 0, n)
        out.append(("stored %d" % n, body, n))
    for a, b in STORED_TWO:
        da, db = (rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (a, b))
        out.append(("stored %d + %d" % (a, b), stored_block(da) + stored_block(db) + b"\0", None))
    for want, have in STORED_TAIL:
        out.append(("stored LEN %d over %d bytes" % (want, have), stored_block(b"xyz"[:have], 0, want), None))
    return out


def refills(body):
    return (len(body) + 255) // 256


@functools.lru_cache(maxsize=None)
def window_bodies():
    """[(name, body)]: dynamic, fixed and stored bodies of 250 to 1,600 compressed bytes (1 to 6 and a
    bit windows of 256), every length residue mod 4 in each kind; and every prefix, at lengths 240 to
    280 and 500 to 530, of one dynamic body: the input ends just before, on and just after a window edge"""
    rng = np.random.default_rng(256)
    out = []
    for kind, level, strategy in (("dynamic", 6, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED)):
        seen, n = set(), 330
        while n < 3400:
            # text with a share of random bytes: the compressed length is about half of n
            data = IC.text(rng, n) + rng.integers(0, 256, n // 16, dtype=np.uint8).tobytes() + IC.text(rng, n // 4)
            body = IC.deflate(data, level, strategy)
            key = (refills(body), len(body) % 4)
            if 250 <= len(body) <= 1600 and key not in seen:
                seen.add(key)
                out.append(("%s %d" % (kind, len(body)), body))
            n += 13
    for n in (244, 245, 246, 247, 506, 763, 1020, 1021, 1277, 1590, 1594):
        out.append(("stored %d" % (n + 6), IC.deflate(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), 0)))
    long_dyn = IC.deflate(IC.text(rng, 3000) + rng.integers(0, 256, 300, dtype=np.uint8).tobytes(), 9)
    assert len(long_dyn) >= 530 and (long_dyn[0] >> 1) & 3 == 2
    for k in list(range(240, 281)) + list(range(500, 531)):
        out.append(("prefix %d" % k, long_dyn[:k]))
    return out
