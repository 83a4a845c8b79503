"""One sparse device arena for parity tests at buffer offsets of 2^31, 2^32 and 2^33
(tests/test_gpu_high_offsets.py, tests/test_gpu_checkers.py).

The arena's base is the d_buf handed to the library; a small wire goes in at a high offset HIGH
and every offset handed in is HIGH + off. An offset truncated to 31 or 32 bits then lands inside
the same allocation: the bug shows as a wrong byte, never as a fault. So next to the 64 guard
bytes on each side of the wire, the low aliases of the window (its addresses mod 2^31 and mod
2^32) carry a sentinel pattern that must come back untouched.

The expected values come from the oracle on the small wire at offset 0; rebase() then adds HIGH
to frame_off and data_off (WEBSOCKET_DATA_OFF_NULL stays).

The first part is numpy only (tests/test_high_arena.py checks it without a GPU); Arena needs torch.
"""
import numpy as np

import dec_cases as D
from oracle_lib import oracle_segments

B31, B32, B33 = 1 << 31, 1 << 32, 1 << 33
ABOVE = B32 + 5                       # one odd placement wholly above 2^32
BOUNDARIES = {"2^31": B31, "2^32": B32, "2^33": B33}
ARENA_BYTES = B33 + (64 << 20)
MIN_FREE = 20 << 30                   # two arenas are 17.2 GB
GUARD = 64
PRE_FILL, PAD_FILL, SLOT_FILL = 0x5C, 0x3C, 0xEE       # as tests/test_gpu_decode_edges.py
DATA_OFF_NULL = 0xFFFFFFFFFFFFFFFF
MODULI = (B31, B32)


def place(boundary, at):
    """HIGH such that wire byte `at` lies at arena offset `boundary`"""
    return boundary - at


def place_pieces(boundary, at):
    """as place(), `at` rounded down to the 16 KiB piece grid: the builders' origin geometry holds"""
    return boundary - at // D.PIECE * D.PIECE


def rebase(desc, high):
    """a copy of oracle descriptors with frame_off and data_off moved by `high`"""
    out = desc.copy()
    with np.errstate(over="ignore"):
        out["frame_off"] += np.uint64(high)
        real = out["data_off"] != np.uint64(DATA_OFF_NULL)
        out["data_off"][real] += np.uint64(high)
    return out


def unrebase(desc, high):
    out = desc.copy()
    with np.errstate(over="ignore"):
        out["frame_off"] -= np.uint64(high)
        real = out["data_off"] != np.uint64(DATA_OFF_NULL)
        out["data_off"][real] -= np.uint64(high)
    return out


def window(high, n):
    """[start, end) of the wire with its guards"""
    return high - GUARD, high + n + GUARD


def _minus(iv, cut):
    a, b = iv
    c, d = cut
    return [x for x in ((a, min(b, c)), (max(a, d), b)) if x[0] < x[1]]


def alias_windows(high, n):
    """where the window's addresses land when cut to 31 or 32 bits: disjoint [start, end) ranges
    below the window, without whatever lies inside the window itself"""
    lo, hi = window(high, n)
    assert lo >= 0 and hi - lo < B31
    out = []
    for m in MODULI:
        if hi <= m:                                       # no address of the window reaches the modulus
            continue
        a = lo % m
        parts = [(a, a + hi - lo)] if a + hi - lo <= m else [(a, m), (0, a + hi - lo - m)]
        for p in parts:
            for q in _minus(p, (lo, hi)):
                out.append(q)
    out.sort()
    merged = []
    for a, b in out:
        if merged and a <= merged[-1][1]:
            merged[-1] = (merged[-1][0], max(b, merged[-1][1]))
        else:
            merged.append((a, b))
    return merged


def sentinel(start, end):
    """the alias fill: depends on the address, so a stray copy of it is seen as well"""
    a = np.arange(start, end, dtype=np.int64)
    return ((a * 37 + (a >> 8) * 11 + 0x61) & 0xFF).astype(np.uint8)


def framed(img, pre=PRE_FILL, pad=PAD_FILL):
    return np.concatenate([np.full(GUARD, pre, np.uint8), img, np.full(GUARD, pad, np.uint8)])


# ---------------------------------------------------------------------------------- byte-exact batch

PAYLOADS = (0, 1, 15, 16, 17, 125, 126, 4096, 70000)
BYTE_EXACT_MF = 4
_byte_exact = []


def byte_exact():
    """(wire, seg_off, seg_len, max_frames, at): 40 segments of 1 to 6 frames, every payload length
    of PAYLOADS masked and unmasked in turn (header lengths 6/2, 8/4, 14/10 in the minimal form, and
    every third round in the next longer form), one truncated segment, one that ends in garbage, one
    that ends in WRAP_HDR; max_frames 4 leaves the fifth and sixth frames unwalked. `at` maps a
    feature's name to the wire offset that a boundary has to fall on to hit it."""
    if _byte_exact:
        return _byte_exact[0]
    rng = np.random.default_rng(4242)
    combos = [(p, m) for p in PAYLOADS for m in (True, False)]
    b = D.Batch(0)
    k = 0
    for i in range(40):
        b.gap(0 if i % 7 == 3 else i * 5 % 13 + 3)
        parts = []
        for _ in range(1 + i % 6):
            plen, masked = combos[k % len(combos)]
            form = None
            if k // len(combos) % 3 == 2 and plen <= 0xFFFF:
                form = 16 if plen < 126 else 64
            parts.append(D.fr(rng, plen, masked=masked, form=form))
            k += 1
        if i == 37:
            parts[-1] = parts[-1][0][:max(1, len(parts[-1][0]) // 2)]
        elif i == 38:
            parts.append(bytes([0x82, 0xFE]) + rng.integers(0, 256, 3, dtype=np.uint8).tobytes())
        elif i == 39:
            parts.append(D.WRAP_HDR + rng.integers(0, 256, 23, dtype=np.uint8).tobytes())
        b.seg(*parts)
    b.gap(9)
    wire, so, sl, mf = b.done(BYTE_EXACT_MF)
    desc, res = oracle_segments(wire.copy(), so, sl, mf)
    at = {}
    for s in range(len(so)):
        for j in range(int(res[s]["n_frames"])):
            d = desc[s * mf + j]
            if int(d["ret"]) <= 0:
                continue
            fo, do, n = int(d["frame_off"]), int(d["data_off"]), int(d["datalen"])
            if int(d["hdrlen"]) == 14 and j and "hdr14:1" not in at:
                for c in range(1, 14):
                    at["hdr14:%d" % c] = fo + c               # between header bytes c - 1 and c
                at["payload_first"], at["payload_last"] = do, do + n - 1
                at["payload_mid_chunk"] = do + 1000 + (7 - (do + 1000)) % 16
            if j and int(d["masked"]) and n >= 16 and "frame_start" not in at and "hdr14:1" in at:
                at["frame_start"] = fo
    s = next(s for s in range(1, len(so)) if so[s] - so[s - 1] - sl[s - 1] >= 3 and sl[s - 1] and sl[s]
             and so[s] > at["frame_start"])
    at["segment_start"], at["gap"] = so[s], so[s] - 2
    _byte_exact.append((wire, so, sl, mf, at))
    return _byte_exact[0]


def header_ats(at):
    return [k for k in at if k.startswith("hdr14:")] + ["segment_start"]


# ---------------------------------------------------------------------------------- the device side

class Arena:
    """a device tensor of ARENA_BYTES, never filled as a whole"""

    def __init__(self, dev):
        import torch
        self.torch, self.dev = torch, dev
        self.t = torch.empty(ARENA_BYTES, dtype=torch.uint8, device=dev)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def sentinel(self, a, b):
        """sentinel(a, b), computed on the device"""
        x = self.torch.arange(a, b, dtype=self.torch.int64, device=self.dev)
        return ((x * 37 + (x >> 8) * 11 + 0x61) & 0xFF).to(self.torch.uint8)

    def framed(self, img, pre=PRE_FILL, pad=PAD_FILL):
        """the image with its guards as a device tensor: what put() and check() take besides numpy"""
        return self.up(framed(np.asarray(img, np.uint8), pre, pad))

    def put(self, high, img, pre=PRE_FILL, pad=PAD_FILL):
        """the image (numpy, or framed() already) with its guards at `high`, sentinels over the
        low aliases; returns the state check() wants"""
        t = img if self.torch.is_tensor(img) else self.framed(img, pre, pad)
        n = t.numel() - 2 * GUARD
        lo, hi = window(high, n)
        assert 0 <= lo and hi <= ARENA_BYTES
        al = alias_windows(high, n)
        for a, b in al:
            self.t[a:b] = self.sentinel(a, b)
        self.t[lo:hi] = t
        return (high, n, pre, pad, al)

    def view(self, high, n):
        """the d_buf to hand in: from the arena's base to the end of the guard after the wire"""
        return self.t[:high + n + GUARD]

    def check(self, state, img, tag=""):
        """the window equals the image (numpy, or framed() already) plus guards, every alias its sentinel"""
        high, n, pre, pad, al = state
        exp = img if self.torch.is_tensor(img) else self.framed(img, pre, pad)
        assert exp.numel() == n + 2 * GUARD
        lo, hi = window(high, n)
        got = self.t[lo:hi]
        if not self.torch.equal(got, exp):
            g, e = got.cpu().numpy(), exp.cpu().numpy()
            bad = np.nonzero(g != e)[0]
            p = int(bad[0]) - GUARD
            zone = "in the guard before" if p < 0 else ("in the guard after" if p >= n else "inside the wire")
            raise AssertionError("%s: %d bytes differ at HIGH 0x%x, first at offset %d (%s): got 0x%02x, want 0x%02x"
                                 % (tag, len(bad), high, p, zone, int(g[bad[0]]), int(e[bad[0]])))
        for a, b in al:
            if not self.torch.equal(self.t[a:b], self.sentinel(a, b)):
                g = self.t[a:b].cpu().numpy()
                bad = np.nonzero(g != sentinel(a, b))[0]
                x = a + int(bad[0])
                raise AssertionError("%s: %d bytes written in the low alias [0x%x, 0x%x) of HIGH 0x%x, first at 0x%x "
                                     "(wire offset %d cut to 31 bits, %d cut to 32)"
                                     % (tag, len(bad), a, b, high, x, (x - high) % B31, (x - high) % B32))


def need_memory(torch, pytest):
    free, _ = torch.cuda.mem_get_info()
    if free < MIN_FREE:
        pytest.skip("the high-offset arenas (2 x 2^33 + 64 MiB) need 20 GiB of free device memory: %.1f GiB free"
                    % (free / 2**30))
