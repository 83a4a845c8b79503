// ws_link.h — the chunk-chain link rule of the raw stream's chunk-parallel walk (ws_stream.hip),
// defined once for every linker: the speculative records and their pools, the emit row, one
// speculative step, and what the records of the chunk the chain enters mean for the chain — a row
// that walks to the stream's end, a row with an owner walk and the next entry, or "walk this chunk".
// A linker only chooses how it looks the records up (scalar loops over the host's copy, one
// wavefront by ballot) and how it carries the chain (a loop, a prefix sum).
//
// The first part is plain C++ — no HIP header, no AMDGPU builtin — so a host compiler can build
// it and a CPU test can hold a scalar model of the whole chunk walk against the oracle
// (tests/test_link_host.py). The second part is device code.
#pragma once
#include "ws_step.h"

#define RW_S0 40          // records per chunk of walks that leave its window (~8-16 true frame starts)
#define RW_S1 8           // ... of walks that end the stream in it
#define RW_SLOTS (RW_S0 + RW_S1)
#define RW_SLAST 4096     // walks that end the stream in the last chunk
#define RW_D 4            // distinct window exits per chunk walked on (phase B owners)
#define RW_MAXSTEPS 65536 // frames of one owner walk at most

struct RwRec {            // phase A: one surviving walk from chunk start + start
    u32 start;
    u32 cs;               // frames consumed | status << 31 (0 left the window, 1 the stream's walk ends)
    u64 exit;             // the next frame start (status 0) or where the walk ended
};

struct RwOwn {            // phase B: the walk from a window exit to the chunk's end
    u64 exit;             // the next frame start (left the chunk) or where the stream's walk ends
    u32 cs;               // frames | status << 31
    u32 dead;             // 1: an implausible header (not the chain)
    u64 over;             // the (stgn+1)-th frame's start when more than stgn frames
    u64 pad;
};

// One emit row per chain chunk: the window prefix [ent, exit_w) by the group walk from frame nf0
// (cnt_w frames), then n_par staged frames of the owner walk in parallel, then the group walk from
// the next frame to the owner's exit (last: to the stream's end — tail, count, result).
struct RwRow {
    u64 ent, exit_w, nf0, cnt_w;
    u64 owner;            // global owner index; ~0ull: the group walk from ent to the stream's end
    u64 n_par, last, cs0; // cs0: the chunk's first byte (staged offsets are relative to it)
};
static_assert(sizeof(RwRow) == 64, "an emit row is eight u64 (table sizing, the host's copy)");

// b23: header bytes 2 and 3 (the top of a 64-bit length, which a real frame leaves zero:
// a random 64-bit length reads as an incomplete frame and would crowd the records)
WS_STEP_FN bool rw_plausible(u32 b0, u32 b1, u32 b23, bool need_mask) {
    const u32 op = b0 & 15u;
    return !(b0 & 0x70u) && (op <= 2u || (op >= 8u && op <= 10u)) && (!need_mask || (b1 & 0x80u)) &&
           ((b1 & 0x7Fu) != 127u || b23 == 0u);
}

// One speculative step over the header (h0, h1) with `avail` (>= 2) bytes left: 0 a frame of
// `fl` bytes, 1 the stream's walk ends here, 2 implausible header (a wrong start)
WS_STEP_FN u32 rw_step_hdr(u64 h0, u64 h1, u64 avail, bool need_mask, u32& fl) {
    fl = 0;
    if (!rw_plausible((u32)h0 & 0xFFu, (u32)(h0 >> 8) & 0xFFu, (u32)(h0 >> 16) & 0xFFFFu, need_mask)) return 2;
    fl = ws_plain_frame_len(ws_parse(h0, h1, avail));
    return fl ? 0u : 1u;
}

// Where the records of (global) chunk c of nchunks lie in the record array, and how many of its
// counts n0 (walks that left the window) and n1 (walks that end the stream) have a slot. The last
// chunk's window lies near the stream's end, where wrong starts read as incomplete frames: its
// walks that end get a pool of their own after every chunk's slots.
struct RwPools {
    u64 i0, i1;           // first record of each kind
    u32 n0, n1;           // valid records of each kind
};
WS_STEP_FN RwPools rw_pools(u64 c, u64 nchunks, u32 n0, u32 n1) {
    const bool lastc = c + 1 == nchunks;
    const u32 cap1 = lastc ? RW_SLAST : RW_S1;
    RwPools p;
    p.i0 = c * RW_SLOTS;
    p.i1 = lastc ? nchunks * RW_SLOTS : c * RW_SLOTS + RW_S0;
    p.n0 = n0 < RW_S0 ? n0 : RW_S0;
    p.n1 = n1 < cap1 ? n1 : cap1;
    return p;
}

// What a lookup found: the record whose start is the chain's entry, and the owner walk of that
// record's window exit
struct RwHit {
    bool found;
    u32 cs;
    u64 exit;
};
struct RwOwnHit {
    u64 oi;               // global owner index, ~0ull: no owner claimed this exit
    u32 cs, dead;
    u64 exit;
};

// scalar lookups (the host linker over its pinned copies, the CPU model)
WS_STEP_FN RwHit rw_find_rec(const RwRec* recs, const RwPools& p, u32 so) {
    RwHit r = {false, 0u, 0ull};
    for (u32 k = 0; k < p.n0 + p.n1; ++k) {
        const RwRec& q = k < p.n0 ? recs[p.i0 + k] : recs[p.i1 + (k - p.n0)];
        if (q.start == so) { r.found = true; r.cs = q.cs; r.exit = q.exit; break; }
    }
    return r;
}
// dx, own: the arrays of every chunk's RW_D claimed exits and their owner walks
WS_STEP_FN RwOwnHit rw_find_own(const unsigned long long* dx, const RwOwn* own, u64 c, u64 exit) {
    RwOwnHit o = {~0ull, 0u, 0u, 0ull};
    for (u32 d = 0; d < RW_D; ++d)
        if (dx[c * RW_D + d] == exit) {
            const RwOwn& w = own[c * RW_D + d];
            o.oi = c * RW_D + d; o.cs = w.cs; o.dead = w.dead; o.exit = w.exit;
            break;
        }
    return o;
}

// an owner walk that ends the chain: the stream's walk ended in it, or it left the stream
WS_STEP_FN bool rw_own_ends(u32 ocs, u64 oexit, u64 len) { return (ocs >> 31) != 0 || oexit >= len; }

// The link decision for the chunk (first byte cs0) the chain enters at `ent` with nfc frames
// before it, from the record at the entry (r.found false: none) and its exit's owner walk:
//   RW_LINK_WALK   no usable record (none, no owner for its exit, a dead owner): the caller walks
//                  the chunk by the step rule
//   RW_LINK_GROUP  row: the group walk from ent to the stream's end (a record that ends in its
//                  window, or max_frames reached inside the window prefix); last
//   RW_LINK_OWNER  row with the owner walk; the chain goes on at `ent` / `nfc` below unless last
// The `last` rule and the n_par clipping live here and nowhere else.
enum { RW_LINK_WALK = 0, RW_LINK_GROUP = 1, RW_LINK_OWNER = 2 };
struct RwLinkOut {
    u32 kind;
    bool last;            // the row ends the chain
    RwRow row;            // (GROUP, OWNER)
    u64 ent, nfc;         // OWNER: the next chunk's entry and the frames before it
};
WS_STEP_FN RwLinkOut rw_link_decide(u64 ent, u64 cs0, u64 nfc, const RwHit& r, const RwOwnHit& o, u32 stgn,
                                    u32 max_frames, u64 len) {
    RwLinkOut d;
    d.kind = RW_LINK_WALK;
    d.last = false;
    d.row.ent = ent; d.row.exit_w = 0; d.row.nf0 = nfc; d.row.cnt_w = 0;
    d.row.owner = ~0ull; d.row.n_par = 0; d.row.last = 1; d.row.cs0 = cs0;
    d.ent = ent;
    d.nfc = nfc;
    if (!r.found) return d;
    const u64 cnt_w = r.cs & 0x7FFFFFFFu;
    if ((r.cs >> 31) || nfc + cnt_w >= max_frames) {                        // ends in the window: group walk
        d.kind = RW_LINK_GROUP;
        d.last = true;
        return d;
    }
    if (o.oi == ~0ull || o.dead) return d;
    const u64 nb = o.cs & 0x7FFFFFFFu;
    d.kind = RW_LINK_OWNER;
    d.last = rw_own_ends(o.cs, o.exit, len) || nfc + cnt_w + nb >= max_frames;
    u64 n_par = nb < stgn ? nb : stgn;
    if (d.last && nfc + cnt_w + n_par > max_frames) n_par = max_frames - nfc - cnt_w;
    d.row.exit_w = r.exit; d.row.cnt_w = cnt_w; d.row.owner = o.oi; d.row.n_par = n_par;
    d.row.last = d.last ? 1ull : 0ull;
    d.ent = o.exit;
    d.nfc = nfc + cnt_w + nb;
    return d;
}

#ifdef __HIPCC__
// ---------------------------------------------------------------------------------------------
// Device part: the lookups by one wavefront (ballot over the lanes, the first match, its fields
// by readlane).
__device__ __forceinline__ u64 rw_readlane64(u64 v, int i) {
    return (u64)(u32)__builtin_amdgcn_readlane((int)(u32)v, i) |
           ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), i) << 32);
}

// One speculative step at pos: 0 frame (pos advanced), 1 the stream's walk ends at pos,
// 2 implausible header (a wrong start)
__device__ __forceinline__ u32 rw_step(uintptr_t origin, u64 len, u64& pos, bool need_mask) {
    if (pos >= len || len - pos < 2) return 1;                               // websocketframe.c:121
    u64 h0, h1;
    ws_load16(origin + pos, h0, h1);
    u32 fl;
    const u32 r = rw_step_hdr(h0, h1, len - pos, need_mask, fl);
    pos += fl;
    return r;
}

// q: the lane's window-exit record of the chunk (recs[p.i0 + lane], lanes < RW_S0; any other
// lane's is not looked at); the walks that end the stream are read here, 64 per round
__device__ __forceinline__ RwHit rw_wave_find_rec(const RwRec& q, const RwRec* __restrict__ recs, const RwPools& p,
                                                  u32 so, u32 lane) {
    RwHit r = {false, 0u, 0ull};
    const u64 m = __ballot(lane < p.n0 && q.start == so);
    if (m) {
        const int i = __builtin_ctzll(m);
        r.found = true;
        r.cs = (u32)__builtin_amdgcn_readlane((int)q.cs, i);
        r.exit = rw_readlane64(q.exit, i);
        return r;
    }
    for (u32 k0 = 0; k0 < p.n1 && !r.found; k0 += 64) {
        RwRec q1 = {};
        if (k0 + lane < p.n1) q1 = recs[p.i1 + k0 + lane];
        const u64 m1 = __ballot(k0 + lane < p.n1 && q1.start == so);
        if (m1) {
            const int i = __builtin_ctzll(m1);
            r.found = true;
            r.cs = (u32)__builtin_amdgcn_readlane((int)q1.cs, i);
            r.exit = rw_readlane64(q1.exit, i);
        }
    }
    return r;
}

// d, w: claimed exit and owner walk (lane & (RW_D - 1)) of chunk c
__device__ __forceinline__ RwOwnHit rw_wave_find_own(unsigned long long d, const RwOwn& w, u64 c, u64 exit, u32 lane) {
    RwOwnHit o = {~0ull, 0u, 0u, 0ull};
    const u64 mo = __ballot(lane < RW_D && d == exit);
    if (mo) {
        const int i = __builtin_ctzll(mo);
        o.oi = c * RW_D + (u64)i;
        o.cs = (u32)__builtin_amdgcn_readlane((int)w.cs, i);
        o.dead = (u32)__builtin_amdgcn_readlane((int)w.dead, i);
        o.exit = rw_readlane64(w.exit, i);
    }
    return o;
}
#endif  // __HIPCC__
