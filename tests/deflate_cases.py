"""Inputs for the deflate tests (test_deflate_host.py, test_gpu_deflate.py): message bodies chosen
for the edges of the rule in util_amd/csrc/ws_deflate.h (groups of 64 positions, matches of 4 to
258 bytes at distances up to 32,768, 8- and 9-bit literals) and a seeded sweep. Expected results
come from deflate_oracle.py (CPython's zlib and the verdict rule), never from here."""
import numpy as np

from inflate_cases import text

GROUP = 64


def rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def far_repeat(dist, n=4):
    """n marker bytes, a filler, the marker again: the repeat lies at distance exactly `dist`. The
    filler has three byte values, none of them the marker's: its 4-byte windows take at most 81 of
    the table's slots, so the marker's slot is still the marker's when the repeat looks it up."""
    marker = bytes([0xF1, 0xF2, 0xF3, 0xF4, 0xF5][:n])
    k = np.arange(dist - n, dtype=np.int64)
    filler = ((k * 2654435761 >> 7) % 3 + 1).astype(np.uint8).tobytes()
    return marker + filler + marker + b"\x05\x06"


def directed_table():
    """(name, body) pairs"""
    t = []
    for n in (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129):
        t.append(("text of %d" % n, text(np.random.default_rng(100 + n), n)))
        t.append(("one value, %d" % n, b"q" * n))
    for n in (257, 258, 259, 260, 516):
        t.append(("one value, %d" % n, b"\x00" * n))
    for n in (3, 4):
        t.append(("%d-byte repeat at distance 32768" % n, far_repeat(32768, n)))
        t.append(("%d-byte repeat at distance 32769" % n, far_repeat(32769, n)))
    t.append(("bytes 144-255", bytes(range(144, 256)) * 3))
    t.append(("bytes 144-255, shuffled", bytes(np.random.default_rng(5).permutation(np.arange(144, 256, dtype=np.uint8)).tobytes()) * 2))
    for n in (1024, 4096, 16384, 70000):
        t.append(("text of %d" % n, text(np.random.default_rng(1), n)))
    t.append(("random 5000", rnd(9, 5000)))
    t.append(("period 3, 1000", b"abc" * 333 + b"a"))
    t.append(("period 65, 700", (bytes(range(65)) * 11)[:700]))
    t.append(("text then random", text(np.random.default_rng(3), 600) + rnd(4, 600)))
    return t


def sweep(count, seed=11, max_len=70000):
    """seeded bodies: text, random bytes, runs and mixtures, lengths 0 to max_len skewed small"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        u = rng.random()
        n = int(rng.integers(0, 200) if u < 0.5 else (rng.integers(0, 3000) if u < 0.93 else rng.integers(0, max_len + 1)))
        kind = k % 5
        if kind == 0:
            b = text(rng, n)
        elif kind == 1:
            b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif kind == 2:
            b = bytes(np.repeat(rng.integers(0, 256, n // 40 + 1, dtype=np.uint8), rng.integers(1, 90, n // 40 + 1)).tobytes())[:n]
        elif kind == 3:
            b = rng.integers(0, 3, n, dtype=np.uint8).tobytes()
        else:
            a = text(rng, n // 2)
            b = a + rng.integers(0, 256, n // 4, dtype=np.uint8).tobytes() + a[:n - n // 2 - n // 4]
        out.append(b)
    return out
