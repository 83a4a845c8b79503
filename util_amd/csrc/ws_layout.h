// ws_layout.h — where things lie in the two workspaces several launchers carve up, each written
// once as byte offsets from a base the caller holds: the piece path's workspace (ws_piece.hip; the
// reassembly and the raw stream lay theirs on top of it) and the scratch of the raw stream's
// chunk-parallel walk (ws_stream.hip).
//
// Plain C++ — no HIP header, no AMDGPU builtin — so a host compiler can build it and a CPU test
// can hold every offset against the formulas written out independently (tests/test_layout_host.py).
#pragma once
#include <stddef.h>

#include "ws_rwplan.h"

static inline size_t ws_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }   // a: a power of two

// Piece workspace: [disorder u32 | nonuni u32 | pad to 16][ptr: npieces u64][nwork: nseg u32]
// [segr: nseg x 16 B, batch form only][items: nseg * max_frames x 16 B]. The batch form places
// segr on 32 B; the stream form (one segment, no segr) pads nwork to 16 B.
struct WsPieceLayout {
    u64 npieces, pbase, c_lo, c_hi;      // pieces touched, the first one, the 16-B chunks [c_lo, c_hi)
    size_t disorder, nonuni, ptr, nwork, segr, items, end;   // segr 0: none; end: the items' end
};
static inline u64 ws_piece_count(u64 lo_org, u64 hi_org) {
    return hi_org > lo_org ? ((hi_org - 1) >> WS_PIECE_SHIFT) - (lo_org >> WS_PIECE_SHIFT) + 1 : 0;
}
static inline WsPieceLayout ws_piece_offsets(u64 npieces, u32 nseg, u32 max_frames, bool with_segr) {
    WsPieceLayout Y = {};
    Y.npieces = npieces;
    Y.nonuni = 4;
    Y.ptr = 16;
    Y.nwork = ws_up(16 + (size_t)npieces * 8, 16);
    Y.items = ws_up(Y.nwork + (size_t)nseg * 4, with_segr ? 32 : 16);
    if (with_segr) {
        Y.segr = Y.items;
        Y.items += (size_t)nseg * 16;
    }
    Y.end = Y.items + (size_t)nseg * max_frames * 16;
    return Y;
}
// segments inside [lo_org, hi_org): byte offsets from the 16-B block the buffer's base lies in
static inline WsPieceLayout ws_piece_layout(u64 lo_org, u64 hi_org, u32 nseg, u32 max_frames, bool with_segr) {
    WsPieceLayout Y = ws_piece_offsets(ws_piece_count(lo_org, hi_org), nseg, max_frames, with_segr);
    Y.pbase = lo_org >> WS_PIECE_SHIFT;
    Y.c_lo = lo_org >> 4;
    Y.c_hi = (hi_org + 15) >> 4;
    return Y;
}
// what a caller allocates for segments spanning `span` bytes wherever they start (batch form)
static inline size_t ws_piece_bytes(u64 span, u32 nseg, u32 max_frames) {
    return ws_piece_offsets((span + 15) / (1ull << WS_PIECE_SHIFT) + 2, nseg, max_frames, true).end + 16;
}

// The raw stream's workspace: the stream form for the one segment [0, len) of a buffer whose base
// lies lead0 (< 16) bytes into its 16-B block (pieces counted from that block: origin 0, so an
// empty stream at an odd base still has its one piece), then the segment's (offset, length) pair.
struct WsStreamLayout { WsPieceLayout piece; size_t seg, bytes; };
static inline WsStreamLayout ws_stream_layout(u64 lead0, u64 len, u32 max_frames) {
    const size_t pws = ws_piece_bytes(len, 1, max_frames);
    return WsStreamLayout{ws_piece_layout(0, len + lead0, 1, max_frames, false), ws_up(pws, 16), pws + 64};
}

// Chunk-walk scratch, every region on 256 B: [head: the device plan, or the host-linked walk's
// 256-B chunk report][nrec: 16 B per chunk][dx: RW_D exits per chunk][recs][own][tab][stg][cand]
// [lk: device plan only]. nrec and dx are zeroed together before every walk; the host-linked walk
// copies [nrec, tab) back in one piece. Nothing reads past a region's own entries (the host-linked
// walk once zeroed 256 B more after dx: no kernel or host loop ever indexed them).
struct RwLayout {
    size_t o_plan, o_nrec, o_dx, o_recs, o_own, o_tab, o_stg, o_cand, o_lk, bytes;
    size_t zero_bytes, back_bytes;   // from o_nrec: nrec + dx; nrec, dx, recs, own (the host's copy back)
};
// plan_bytes 0: host-linked (no plan, no link table, one emit row per chunk); else the device
// plan's size, link_bytes per chunk of link table and two emit rows to spare
static inline RwLayout rw_carve(u64 chunks, u64 stg_words, u64 cand_words, size_t plan_bytes, size_t link_bytes) {
    RwLayout L;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += ws_up(bytes, 256); return at; };
    L.o_plan = take(plan_bytes ? plan_bytes : 256);
    L.o_nrec = take((size_t)chunks * 16);
    L.o_dx = take((size_t)chunks * RW_D * 8);
    L.zero_bytes = o - L.o_nrec;
    L.o_recs = take((size_t)(chunks * RW_SLOTS + RW_SLAST) * sizeof(RwRec));
    L.o_own = take((size_t)chunks * RW_D * sizeof(RwOwn));
    L.back_bytes = o - L.o_nrec;
    L.o_tab = take((size_t)(chunks + (plan_bytes ? 2 : 0)) * sizeof(RwRow));
    L.o_stg = take((size_t)stg_words * 4);
    L.o_cand = take((size_t)cand_words * 8);
    L.o_lk = take((size_t)chunks * link_bytes);
    L.bytes = o;
    return L;
}

// A device-planned call's scratch is sized from the stream length alone (a captured call cannot
// read its sample): the smallest chunk that keeps the chunk count under RW_CAP_CHUNKS, and caps
// for the candidate and staging lists.
struct RwDevLayout {
    u64 cmin, nch_cap, cand_cap, stg_cap;
    RwLayout at;
};
static inline RwDevLayout rw_dev_layout(u64 len, size_t plan_bytes, size_t link_bytes) {
    RwDevLayout L;
    L.cmin = RW_CMIN;
    while ((len + L.cmin - 1) / L.cmin + 2 > RW_CAP_CHUNKS) L.cmin <<= 1;
    L.nch_cap = (len + L.cmin - 1) / L.cmin + 2;
    const u64 cand = L.nch_cap * (RW_HMAX / 32), stg = L.nch_cap * RW_D * RW_CAP_STGN;
    L.cand_cap = cand < len / 1024 + 65536 ? cand : len / 1024 + 65536;
    L.stg_cap = stg < len / 256 + 65536 ? stg : len / 256 + 65536;
    L.at = rw_carve(L.nch_cap, L.stg_cap, L.cand_cap, plan_bytes, link_bytes);
    return L;
}
