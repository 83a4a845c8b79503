// ws_rwplan.h — the geometry of the raw stream's chunk-parallel walk (ws_stream.hip), written
// once: from the sample's end P1, the stream's length, the sample's mean wire frame and the longest
// frame seen, the chunk size C, the window H, the one to three parts of a split walk (each a chunk
// grid of its own), their chunk counts and the bases and sizes of their staging and candidate
// lists. The device plan (ws_rw_plan_kernel: captured and device-planned eager calls) and the
// host-linked eager walk (stream_rw 2) take it from here and nowhere else.
//
// Plain C++ — no HIP header, no AMDGPU builtin — so a host compiler can build it and a CPU test
// can hold it against an independent model (tests/test_rwplan_host.py).
#pragma once
#include "ws_link.h"

#define RW_CMAX (16ull << 20)
#define RW_CMIN (64ull << 10)
#define RW_HMAX (128u << 10)
#define RW_HMIN (4u << 10)
#define RW_SAMPLE (256ull << 10)
#define RW_STG 4096       // the host-linked walk's largest staging list per owner (frame offsets)
#define RW_MIN (512ull << 10)     // streams shorter than this after the passes: one wavefront walks
#define RW_MIN_FRAMES 256         // ... and, after the sample, fewer frames than this (by the mean)
#define RW_CAP_CHUNKS 32768u   // a device-planned call's chunk-count cap (the smallest chunk follows)
#define RW_CAP_STGN 1024u      // ... and staging per owner
#define RW_NP 3           // parts of a split walk at most

// the smallest lo << k that is >= x, at most hi (lo when hi < lo)
WS_STEP_FN u64 rw_pow2_clamp(u64 x, u64 lo, u64 hi) {
    u64 v = lo;
    while (v < x && v < hi) v <<= 1;
    return v;
}

// The window at each chunk's start must hold a frame start of the chain: any window longer
// than every frame does. 4 mean frames or the longest frame seen + 4 KiB, whichever is
// larger, in 4 KiB steps, within [RW_HMIN, min(C / 2, RW_HMAX)] (round 3: 8 mean frames
// rounded up to a power of two; cfg3 128 -> 92 KiB, stream 8.32-8.36 -> 8.19 ms eager,
// profiles/r04_stream_rw_ab.log)
WS_STEP_FN u32 rw_window(u64 mean, u32 maxlen, u64 C) {
    // (round 5: 0, 2 or 4 mean frames measured the same on one buffer, R1 unchanged at 247 us)
    const u64 hi = C / 2 < RW_HMAX ? C / 2 : RW_HMAX;
    u64 h = mean * 4 > (u64)maxlen + 4096 ? mean * 4 : (u64)maxlen + 4096;
    h = (h + 4095) & ~4095ull;
    return (u32)(h < RW_HMIN ? RW_HMIN : (h > hi ? hi : h));
}

// the sample [P, P1) held `frames` frames: its mean wire frame
WS_STEP_FN u64 rw_sample_mean(u64 P, u64 P1, u64 frames) { return frames ? (P1 - P) / frames : (P1 - P); }

// the rest after the sample is too short for chunks (fewer than RW_MIN_FRAMES mean frames): one wavefront walks it
WS_STEP_FN bool rw_short_rest(u64 P1, u64 len, u64 mean) { return (len - P1) / (mean ? mean : 1) < RW_MIN_FRAMES; }

struct RwPart {
    u64 P;                // the part's chunk grid origin
    u64 C;                // its chunk bytes
    u32 H, n, cbase, capc; // window bytes, chunks, first global chunk, candidates per chunk
    u32 stgn, pad;        // staging per owner
    u64 stg_base, cand_base;  // where its staging and candidate lists start (entries)
};

// what the device plan is made from
struct RwPlanIn {
    u64 P1, len;          // the rest of the stream [P1, len), P1 < len
    u64 mean;             // the sample's mean wire frame
    u32 longest;          // the longest frame seen: the sample's or the previous walk's on this stream
    u64 cmin, cmax;       // the chunk's bounds (cmin: the layout's, at least RW_CMIN; cmax: the option's)
    u32 nchunks_cap;      // the scratch's caps: chunks, candidate entries, staging entries
    u64 cand_cap, stg_cap; // (each holds at least RW_NP chunks of the smallest lists, or no C fits)
    u64 split_x[RW_NP - 1];   // the first stream byte K2's second / third launch own; 0: no such cut
    u32 shift[RW_NP - 1];     // part 0's / a middle part's chunks: C >> shift
};
struct RwGeom {
    RwPart pt[RW_NP];     // parts past nparts are empty: n 0, P = len, bases where the lists end
    u32 nparts, nchunks;  // nchunks: the parts' chunks together
};

// The rest of the stream after the sample as one to RW_NP parts. Part k < the last ends at the
// first of its chunk starts at or past split_x[k] (the stream's end if that lies past it; a cut at
// or before the part's origin leaves the part empty); a cut of 0 or at or past len ends the list.
// Part 0's chunks are C >> shift[0], a middle part's C >> shift[1] — a power of two of at least
// twice the window a frame start needs, within [RW_CMIN, C] — the last part's C, where C =
// pow2(1024 mean) within [max(cmin, RW_CMIN), max(cmin, cmax)], doubled until the chunk count and
// the smallest lists (64 entries) fit the caps. Staging per owner: pow2(2 C_k / mean) within
// [256, RW_CAP_STGN]; candidates per chunk: H_k / 32; both halved part by part (never below 64)
// while their totals exceed the caps.
WS_STEP_FN RwGeom rw_plan_geometry(const RwPlanIn& in) {
    const u64 P1 = in.P1, len = in.len, mean = in.mean;
    u64 C = rw_pow2_clamp(mean * 1024, in.cmin > RW_CMIN ? in.cmin : RW_CMIN, in.cmin > in.cmax ? in.cmin : in.cmax);
    const u64 hneed = rw_window(mean, in.longest, 4 * (u64)RW_HMAX);
    u64 Pk[RW_NP], Ck[RW_NP], nk[RW_NP];
    u32 np = 1;
    for (;;) {
        u64 B = P1, tot = 0;
        np = 0;
        for (u32 k = 0; k < RW_NP; ++k) {
            const bool lastp = k + 1 == RW_NP || !in.split_x[k] || in.split_x[k] >= len;
            u64 Cx = C;
            if (!lastp) {
                const u64 want = (C >> in.shift[k]) > 2 * hneed ? (C >> in.shift[k]) : 2 * hneed;
                Cx = rw_pow2_clamp(want, RW_CMIN, C);
            }
            u64 E = len;
            if (!lastp) {
                E = in.split_x[k] > B ? B + (in.split_x[k] - B + Cx - 1) / Cx * Cx : B;
                if (E >= len) E = len;
            }
            Pk[k] = B; Ck[k] = Cx; nk[k] = E > B ? (E - B + Cx - 1) / Cx : 0;
            tot += nk[k];
            ++np;
            B = E;
            if (lastp || E >= len) break;
        }
        // fit the caps (cmin makes the chunk count fit; the smallest staging and candidate lists too)
        if (tot <= in.nchunks_cap && tot * RW_D * 64 <= in.stg_cap && tot * 64 <= in.cand_cap) break;
        C <<= 1;
    }
    u64 Hk[RW_NP], stgk[RW_NP], capk[RW_NP];
    for (u32 k = 0; k < np; ++k) {
        Hk[k] = rw_window(mean, in.longest, Ck[k]);
        stgk[k] = rw_pow2_clamp(2 * Ck[k] / (mean ? mean : 1), 256, RW_CAP_STGN);
        capk[k] = Hk[k] / 32;
    }
    for (;;) {                                                               // shrink staging / candidates to the caps
        u64 stg_need = 0, cand_need = 0;
        bool can = false;
        for (u32 k = 0; k < np; ++k) {
            stg_need += nk[k] * RW_D * stgk[k];
            cand_need += nk[k] * capk[k];
            can = can || stgk[k] > 64 || capk[k] > 64;
        }
        if ((stg_need <= in.stg_cap && cand_need <= in.cand_cap) || !can) break;
        for (u32 k = 0; k < np; ++k) {
            // (never below 64: a window of 12 KiB has 384 candidates, and 96 halves to 48, under the
            // smallest list the chunk size was fitted for)
            if (stg_need > in.stg_cap && stgk[k] > 64) stgk[k] = stgk[k] >> 1 > 64 ? stgk[k] >> 1 : 64;
            if (cand_need > in.cand_cap && capk[k] > 64) capk[k] = capk[k] >> 1 > 64 ? capk[k] >> 1 : 64;
        }
    }
    RwGeom G;
    u64 cb = 0, sb = 0, cdb = 0;
    for (u32 k = 0; k < RW_NP; ++k) {
        RwPart& t = G.pt[k];
        t.pad = 0;
        if (k < np) {
            t.P = Pk[k]; t.C = Ck[k]; t.H = (u32)Hk[k]; t.n = (u32)nk[k]; t.cbase = (u32)cb; t.capc = (u32)capk[k];
            t.stgn = (u32)stgk[k]; t.stg_base = sb; t.cand_base = cdb;
            cb += nk[k]; sb += nk[k] * RW_D * stgk[k]; cdb += nk[k] * capk[k];
        } else {
            t.P = len; t.C = C; t.H = RW_HMIN; t.n = 0; t.cbase = (u32)cb; t.capc = 64; t.stgn = 64;
            t.stg_base = sb; t.cand_base = cdb;
        }
    }
    G.nchunks = (u32)cb;
    G.nparts = np;
    return G;
}

// The host-linked eager walk (stream_rw 2): one part, chunks of pow2(1024 mean) within
// [RW_CMIN, cmax], windows of pow2(8 mean) within [RW_HMIN, min(C / 2, RW_HMAX)] (round 2's rule:
// no longest frame, no 4 KiB steps), staging pow2(2 C / mean) within [256, RW_STG]
struct RwHostGeom {
    u64 C, nchunks;
    u32 H, stgn, capc;
};
WS_STEP_FN RwHostGeom rw_host_geometry(u64 P1, u64 len, u64 mean, u64 cmax) {
    RwHostGeom G;
    G.C = rw_pow2_clamp(mean * 1024, RW_CMIN, cmax);
    G.H = (u32)rw_pow2_clamp(mean * 8, RW_HMIN, G.C / 2 < RW_HMAX ? G.C / 2 : RW_HMAX);
    G.nchunks = (len - P1 + G.C - 1) / G.C;
    G.stgn = (u32)rw_pow2_clamp(2 * G.C / (mean ? mean : 1), 256, RW_STG);
    G.capc = G.H / 32;                                                       // candidates: 1/32 of a window
    return G;
}
