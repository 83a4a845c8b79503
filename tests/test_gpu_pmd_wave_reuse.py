"""What a wavefront of the deflate and inflate kernels carries from one item to the next. Both launch
a fixed grid (BLOCKS_PER_CU x WAVES waves per CU) and stride over it, so item q runs on the wave that
ran q - G, G the grid's wave count: only a batch of more than G items takes the loop's second trip.
These batches have 2.3 G items and a bit, of kinds laid out so that every ordered pair (A, then B on the
same wave) occurs: the LDS hash table cleared only up to the new message's size, the staging words,
`skip`, the block tables and header scratch, the window base. Deflate bit for bit against the host
twin, inflate against the sequential model, as test_gpu_deflate.py and test_gpu_inflate.py."""
import math
import os
import re

import numpy as np
import pytest

import deflate_oracle as DO
import inflate_cases as IC
import inflate_oracle as O
import test_gpu_deflate as TD
import test_gpu_inflate as TI
from util_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def grid_waves(dev, source, prefix):
    """the fixed grid's wave count: compute units x PREFIX_BLOCKS_PER_CU x PREFIX_WAVES of the kernel's source"""
    text = open(os.path.join(_lib.REPO, "util_amd", "csrc", source)).read()
    per_cu = int(re.search(r"#define %s_BLOCKS_PER_CU (\d+)" % prefix, text).group(1))
    waves = int(re.search(r"#define %s_WAVES (\d+)" % prefix, text).group(1))
    return torch.cuda.get_device_properties(dev).multi_processor_count * per_cu * waves


def layout(count, G, K):
    """a kind for every item. With r = a + K * b the place in the first trip, the items r and r + G
    are of kinds a * m and a * m + b (mod K): every ordered pair in every K * K places; the third trip
    pairs them up differently again. The stride m, coprime to K, changes every K * K places, so no kind
    has the same neighbour everywhere"""
    q = np.arange(count)
    r, t = q % G, q // G
    strides = np.array([m for m in range(1, K) if math.gcd(m, K) == 1])
    a = (r % K) * strides[(r // (K * K)) % len(strides)]
    return (a + t * ((r // K) % K) + (t >= 2)) % K


def pairs(kinds, G):
    return set(zip(kinds[:-G].tolist(), kinds[G:].tolist()))


# ---------------------------------------------------------------------------------- deflate

LONG, SHORT, MID, RUN, RANDOM, BELOW, SKIPPED, PAST, RANGE = range(9)
MIN_LEN = 32


def deflate_batch(G, mm=3):
    """(src, per connection its live entries, the slots' kinds) of a batch of 2.3 G slots and a bit"""
    nseg = (math.ceil(2.3 * G) + 5 + mm - 1) // mm
    count = nseg * mm
    assert count > 2 * G
    rng = np.random.default_rng(23)
    # one text stream for the long, middle and short texts: whatever a long message left in the table
    # points at bytes that a short one cut from the same stream may well repeat
    stream = IC.text(rng, 1 << 16)
    noise = rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    runs = b"".join(bytes([v]) * 1200 for v in (0, 7, 0x90, 0xFF))
    src = np.frombuffer(stream + noise + runs, np.uint8).copy()
    n0, r0 = len(stream), len(stream) + len(noise)
    kinds = layout(count, G, 9)
    for s in range(nseg):                                 # a slot past the count takes the slots behind it along
        for i in range(mm):
            if kinds[s * mm + i] == PAST:
                kinds[s * mm + i:(s + 1) * mm] = PAST
                break
    assert pairs(kinds, G) == {(a, b) for a in range(9) for b in range(9)}
    assert (kinds == LONG).mean() <= 1 / 8
    conns = []
    for s in range(nseg):
        lst = []
        for i in range(mm):
            k = int(kinds[s * mm + i])
            if k == PAST:
                break
            if k in (LONG, SHORT, MID, BELOW):
                lo, hi = {LONG: (2500, 3001), SHORT: (40, 201), MID: (300, 1001), BELOW: (1, MIN_LEN)}[k]
                n = int(rng.integers(lo, hi))
                lst.append((int(rng.integers(0, n0 - n)), n, 1))
            elif k == RUN:
                n = int(rng.integers(40, 1201))
                lst.append((r0 + 1200 * int(rng.integers(0, 4)) + int(rng.integers(0, 1201 - n)), n, 2))
            elif k == RANDOM:
                n = int(rng.integers(MIN_LEN, 1500))
                lst.append((n0 + int(rng.integers(0, len(noise) - n)), n, 2))
            elif k == SKIPPED:
                lst.append((len(src) + 9, 1 << 44, DO.SKIP))
            else:
                lst.append((len(src) - 3, 10, 1))
        conns.append(lst)
    return src, conns, kinds


def test_deflate_second_and_third_item_of_every_wave(dev):
    G = grid_waves(dev, "ws_deflate.hip", "DEF")
    src, conns, kinds = deflate_batch(G)
    count = len(kinds)
    c = TD.Call(dev, src, conns, min_len=MIN_LEN, max_msgs=3, nmsg=[len(cn) for cn in conns])
    rec = c.records()
    for k, want in ((LONG, DO.DEFLATED), (SHORT, DO.DEFLATED), (MID, DO.DEFLATED), (RUN, DO.DEFLATED), (RANDOM, DO.PLAIN),
                    (BELOW, DO.PLAIN), (SKIPPED, DO.SKIPPED), (RANGE, DO.ERR_RANGE)):
        assert (rec["status"][kinds == k] == want).mean() > 0.7, (k, want)
    hbits = {(int(n) - 1).bit_length() for n in c.msg_np["len"][np.isin(kinds, (LONG, SHORT, MID))]}
    assert {min(max(b, 8), 11) for b in hbits} == {8, 9, 10, 11}
    c.run()
    c.check("deflate, %d slots over %d waves" % (count, G))


# ---------------------------------------------------------------------------------- inflate

DYN, FIX, STORED, HAND, TRUNC, BAD, SKIP, ZERO = range(8)
HEADER_ERRORS = ("repeat with nothing to repeat", "repeat past HLIT + HDIST", "no code for symbol 256",
                 "over-subscribed code-length set", "incomplete code-length set", "over-subscribed literal/length set",
                 "over-subscribed distance set", "incomplete literal/length set", "incomplete distance set", "HLIT 287")


def inflate_pools():
    """kind -> bodies. BAD: every body fails inside a dynamic block's header; TRUNC: the input ends there"""
    rng = np.random.default_rng(29)
    hand = {name: body for name, body, _ in IC.hand_built()}
    pools = {DYN: [IC.deflate(IC.text(rng, int(n)), 9) for n in rng.integers(260, 700, 8)],
             FIX: [IC.deflate(IC.text(rng, int(n)), 6, 4) for n in rng.integers(20, 400, 8)],
             STORED: [IC.deflate(rng.integers(0, 256, int(n), dtype=np.uint8).tobytes(), 0) for n in rng.integers(1, 300, 8)],
             HAND: [b for name, b in hand.items() if "single-code" in name or "empty code-length" in name or
                    "incomplete distance set" in name or "incomplete literal/length set" in name or "no distance code" in name],
             BAD: [hand[name] for name in HEADER_ERRORS]}
    pools[TRUNC] = [pools[DYN][k % 8][:cut] for k, cut in enumerate((3, 9, 11, 13, 16, 19, 22, 25))]
    assert all((b[0] >> 1) & 3 == 2 for b in pools[DYN] + pools[BAD] + pools[HAND]) and len(pools[HAND]) >= 8
    assert all((b[0] >> 1) & 3 == 1 for b in pools[FIX])
    assert all(O.inflate_one(b)[0] == O.ERR_DATA for b in pools[BAD])
    assert all(O.inflate_one(b) == (O.OK, b"") for b in pools[TRUNC])
    return pools


def inflate_batch(G):
    """(src, connections, their counts, their rooms, their kinds) of a batch of 2.3 G connections and a bit"""
    count = math.ceil(2.3 * G) + 5
    assert count > 2 * G
    kinds = layout(count, G, 8)
    got = pairs(kinds, G)
    assert got == {(a, b) for a in range(8) for b in range(8)}
    assert {(BAD, FIX), (BAD, DYN), (TRUNC, FIX), (TRUNC, DYN)} <= got
    pools = inflate_pools()
    order = sorted(pools)
    flat = [b for k in order for b in pools[k]]
    src, spans = TI.place(flat, [(5 * j) % 16 for j in range(len(flat))])
    first = {k: sum(len(pools[j]) for j in order if j < k) for k in order}
    rng = np.random.default_rng(31)
    conns, nmsg, caps = [], [], []
    for q in range(count):
        k = int(kinds[q])
        if k in pools:
            j = first[k] + int(rng.integers(0, len(pools[k])))
            conns.append([spans[j] + (O.RAW,)])
            caps.append(len(O.inflate_one(flat[j])[1]))
        else:
            conns.append([(len(src) + 5, 1 << 40, O.SKIP)])
            caps.append(0)
        nmsg.append(0 if k == ZERO else 1)
    return src, conns, nmsg, caps, kinds


def test_inflate_second_and_third_item_of_every_wave(dev):
    G = grid_waves(dev, "ws_inflate.hip", "INF")
    src, conns, nmsg, caps, kinds = inflate_batch(G)
    count = len(kinds)
    c = TI.Call(dev, src, conns, caps=caps, nmsg=nmsg, odd=True)
    st = c.exp[1]["status"]
    assert (st[kinds == BAD] == O.ERR_DATA).all() and (st[(kinds != BAD) & (kinds != HAND)] == O.OK).all()
    assert (c.exp[1]["out_len"][np.isin(kinds, (DYN, FIX, STORED))] > 0).all()
    c.run()
    c.check("inflate, %d connections over %d waves" % (count, G))
