// A thin C shim over util_amd/csrc/ws_layout.h (the piece workspace's layout and the chunk-walk
// scratch's) for tests/test_layout_host.py, which writes the expected offsets out on its own.
#include "../../util_amd/csrc/ws_layout.h"

#include <stdint.h>

static void put_piece(const WsPieceLayout& Y, uint64_t* o) {
    o[0] = Y.npieces; o[1] = Y.pbase; o[2] = Y.c_lo; o[3] = Y.c_hi; o[4] = Y.disorder; o[5] = Y.nonuni; o[6] = Y.ptr;
    o[7] = Y.nwork; o[8] = Y.segr; o[9] = Y.items; o[10] = Y.end;
}

// n rows of in[5] = lo_org, hi_org, nseg, max_frames, with_segr -> out[11] = npieces, pbase, c_lo, c_hi,
// disorder, nonuni, ptr, nwork, segr, items, end
extern "C" void ws_layout_piece(uint64_t n, const uint64_t* in, uint64_t* out) {
    for (uint64_t i = 0; i < n; ++i, in += 5, out += 11)
        put_piece(ws_piece_layout(in[0], in[1], (u32)in[2], (u32)in[3], in[4] != 0), out);
}

// n rows of in[3] = span, nseg, max_frames -> out[1] = the bytes a caller allocates
extern "C" void ws_layout_piece_bytes(uint64_t n, const uint64_t* in, uint64_t* out) {
    for (uint64_t i = 0; i < n; ++i, in += 3) out[i] = ws_piece_bytes(in[0], (u32)in[1], (u32)in[2]);
}

// n rows of in[3] = lead0, len, max_frames -> out[13] = the piece layout, then seg, bytes
extern "C" void ws_layout_stream(uint64_t n, const uint64_t* in, uint64_t* out) {
    for (uint64_t i = 0; i < n; ++i, in += 3, out += 13) {
        const WsStreamLayout S = ws_stream_layout(in[0], in[1], (u32)in[2]);
        put_piece(S.piece, out);
        out[11] = S.seg;
        out[12] = S.bytes;
    }
}

static void put_walk(const RwLayout& L, uint64_t* o) {
    o[0] = L.o_plan; o[1] = L.o_nrec; o[2] = L.o_dx; o[3] = L.o_recs; o[4] = L.o_own; o[5] = L.o_tab; o[6] = L.o_stg;
    o[7] = L.o_cand; o[8] = L.o_lk; o[9] = L.bytes; o[10] = L.zero_bytes; o[11] = L.back_bytes;
}

// out[12] = o_plan, o_nrec, o_dx, o_recs, o_own, o_tab, o_stg, o_cand, o_lk, bytes, zero_bytes, back_bytes
extern "C" void ws_layout_carve(uint64_t chunks, uint64_t stg_words, uint64_t cand_words, uint64_t plan_bytes,
                                uint64_t link_bytes, uint64_t* out) {
    put_walk(rw_carve(chunks, stg_words, cand_words, plan_bytes, link_bytes), out);
}

// out[16] = cmin, nch_cap, cand_cap, stg_cap, then the carve's twelve
extern "C" void ws_layout_device(uint64_t len, uint64_t plan_bytes, uint64_t link_bytes, uint64_t* out) {
    const RwDevLayout L = rw_dev_layout(len, plan_bytes, link_bytes);
    out[0] = L.cmin; out[1] = L.nch_cap; out[2] = L.cand_cap; out[3] = L.stg_cap;
    put_walk(L.at, out + 4);
}

// out[] = the constants and record sizes the test's own formulas need to be told
extern "C" void ws_layout_consts(uint64_t* out) {
    out[0] = WS_PIECE_SHIFT; out[1] = RW_D; out[2] = RW_SLOTS; out[3] = RW_SLAST; out[4] = sizeof(RwRec); out[5] = sizeof(RwOwn);
    out[6] = sizeof(RwRow); out[7] = RW_CMIN; out[8] = RW_CAP_CHUNKS; out[9] = RW_HMAX; out[10] = RW_CAP_STGN; out[11] = RW_MIN;
}
