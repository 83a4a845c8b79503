"""An exact-integer model of the geometry of the raw stream's chunk-parallel walk, written from
DESIGN §3.5 (not from util_amd/csrc/ws_rwplan.h, which tests/test_rwplan_host.py holds against it):
the sample's mean, the chunk C, the window H, the parts of a split walk and their lists. Python
integers only, closed forms where the header loops. Shared by the header's CPU test, the case
builders of tests/stream_cases.py and the GPU test that reads a call's plan back."""
from collections import namedtuple

KIB = 1 << 10
CMIN, CMAX = 64 * KIB, 16 << 20            # a chunk: a power of two of 64 KiB .. 16 MiB
HMIN, HMAX, HSTEP = 4 * KIB, 128 * KIB, 4 * KIB
SAMPLE = 256 * KIB                         # the sample: up to the first frame start at or past P + 256 KiB
MIN_STREAM = 512 * KIB                     # shorter streams never take the chunk walk
MIN_FRAMES = 256                           # ... nor a rest of fewer mean frames than this
NP = 3                                     # parts at most
OWNERS = 4                                 # owner walks (distinct window exits) per chunk
STGN_MIN, STGN_DEV, STGN_HOST = 256, 1024, 4096
LIST_MIN = 64                              # the smallest staging / candidate list
CAP_CHUNKS = 32768                         # a device-planned call's chunk cap
PIECE = 16384                              # the unmask's piece (the split options count pieces)

Part = namedtuple("Part", "P C H n cbase capc stgn stg_base cand_base")
Geom = namedtuple("Geom", "parts nparts nchunks")


def ceil_div(a, b):
    return -(-a // b)


def pow2_from(x, lo, hi):
    """the smallest lo * 2^k that is >= x, never more than hi (hi = lo * 2^j; lo when hi < lo)"""
    if hi <= lo or x <= lo:
        return lo
    assert hi % lo == 0 and (hi // lo) & (hi // lo - 1) == 0
    k = (ceil_div(x, lo) - 1).bit_length()
    return min(lo << k, hi)


def mean_of(P, P1, frames):
    return (P1 - P) // frames if frames else P1 - P


def short_rest(P1, length, mean):
    return (length - P1) // max(mean, 1) < MIN_FRAMES


def window(mean, longest, C):
    """4 mean frames or the longest frame seen + 4 KiB, in 4 KiB steps, within [4 KiB, min(C/2, 128 KiB)]"""
    want = ceil_div(max(4 * mean, longest + 4096), HSTEP) * HSTEP
    return max(HMIN, min(want, C // 2, HMAX))


def _parts_for(P1, length, C, hneed, cuts):
    """[(origin, chunk, chunks)]: a part before a cut ends at its first chunk start at or past the cut"""
    out, B = [], P1
    for x, shift in cuts:
        Cx = pow2_from(max(C >> shift, 2 * hneed), CMIN, C)
        E = B if x <= B else min(length, B + ceil_div(x - B, Cx) * Cx)
        out.append((B, Cx, ceil_div(E - B, Cx)))
        B = E
        if E >= length:
            return out
    out.append((B, C, ceil_div(length - B, C)))
    return out


def device_plan(P1, length, mean, longest, cmin, cmax, nchunks_cap, cand_cap, stg_cap, split_x=(0, 0), shifts=(0, 0)):
    assert P1 < length
    cuts = []
    for x, s in zip(split_x, shifts):          # the first cut that is none (0, or at or past the end) ends the list
        if x == 0 or x >= length:
            break
        cuts.append((x, s))
    lo = max(cmin, CMIN)
    C = pow2_from(1024 * mean, lo, max(cmin, cmax))
    hneed = window(mean, longest, 4 * HMAX)    # the window a frame start needs, whatever the chunk
    while True:
        ps = _parts_for(P1, length, C, hneed, cuts)
        tot = sum(n for _, _, n in ps)
        if tot <= nchunks_cap and tot * OWNERS * LIST_MIN <= stg_cap and tot * LIST_MIN <= cand_cap:
            break
        C *= 2
    H = [window(mean, longest, c) for _, c, _ in ps]
    stgn = [pow2_from(2 * c // max(mean, 1), STGN_MIN, STGN_DEV) for _, c, _ in ps]
    capc = [h // 32 for h in H]
    ns = [n for _, _, n in ps]
    while sum(n * OWNERS * s for n, s in zip(ns, stgn)) > stg_cap and any(s > LIST_MIN for s in stgn):
        stgn = [max(LIST_MIN, s // 2) for s in stgn]
    while sum(n * c for n, c in zip(ns, capc)) > cand_cap and any(c > LIST_MIN for c in capc):
        capc = [max(LIST_MIN, c // 2) for c in capc]
    parts, cb, sb, db = [], 0, 0, 0
    for k in range(NP):
        if k < len(ps):
            parts.append(Part(ps[k][0], ps[k][1], H[k], ns[k], cb, capc[k], stgn[k], sb, db))
            cb, sb, db = cb + ns[k], sb + ns[k] * OWNERS * stgn[k], db + ns[k] * capc[k]
        else:
            parts.append(Part(length, C, HMIN, 0, cb, LIST_MIN, LIST_MIN, sb, db))
    return Geom(parts, len(ps), cb)


def host_plan(P1, length, mean, cmax):
    """the host-linked walk (stream_rw 2): (C, H, nchunks, stgn, capc); H = pow2(8 mean)"""
    C = pow2_from(1024 * mean, CMIN, cmax)
    H = pow2_from(8 * mean, HMIN, min(C // 2, HMAX))
    return C, H, ceil_div(length - P1, C), pow2_from(2 * C // max(mean, 1), STGN_MIN, STGN_HOST), H // 32


# ---- what the library passes for a stream of `length` bytes at buffer phase `lead` (address mod 16)

def layout_caps(length):
    """(cmin, nchunks_cap, cand_cap, stg_cap) of a device-planned call's scratch"""
    cmin = CMIN
    while ceil_div(length, cmin) + 2 > CAP_CHUNKS:
        cmin *= 2
    cap = ceil_div(length, cmin) + 2
    return cmin, cap, min(cap * (HMAX // 32), length // 1024 + 65536), min(cap * OWNERS * STGN_DEV, length // 256 + 65536)


def split_bytes(length, lead, split, split2):
    """the first stream byte of K2's second / third launch (0: none), from the options in 256ths of the pieces"""
    npieces = ((length + lead - 1) // PIECE) + 1 if length + lead else 0
    if not (0 < split < 256) or npieces < 3:
        return (0, 0)
    p = [max(1, npieces * split // 256)]
    if split < split2 < 256:
        p1 = npieces * split2 // 256
        if p[0] < p1 < npieces:
            p.append(p1)
    x = [q * PIECE - lead for q in p]
    return (x[0], x[1] if len(x) > 1 else 0)


def call_plan(P1, length, mean, longest, lead=0, split=8, split2=48, c0=3, c1=2, cmax_log=22):
    """the plan of an eager device-planned call with these option values"""
    cmin, ncap, ccap, scap = layout_caps(length)
    xs = split_bytes(length, lead, split, split2)
    cmax = min((1 << cmax_log) << (1 if xs[0] else 0), CMAX)     # a split walk's last part: twice the usual largest
    return device_plan(P1, length, mean, longest, cmin, cmax, ncap, ccap, scap, xs, (c0, c1) if xs[0] else (0, 0))
