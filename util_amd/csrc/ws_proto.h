// ws_proto.h — the framing and sequencing rule of the protocol check (RFC 6455 5.2, 5.4, 5.5,
// 7.4; include/wsframe_amd_proto.h), defined once: a frame's code given what came before it on
// its connection, the summary of a run of frames and how two summaries combine, and the
// per-connection state word. Plain C++ — no HIP header, no AMDGPU builtin — so the kernels
// (ws_proto.hip), the host step (websocketframeProtoStepHost) and a host driver
// (tests/c/proto_host.cpp, tests/test_proto_host.py) build the same text and cannot drift apart.
//
// Scan form. What a frame needs from the frames before it is (open, bytes, closed):
//   open    !is_fin of the last live data frame, else the incoming OPEN bit;
//   bytes   the datalen sum of the live data frames after the last live data frame with FIN,
//           plus the incoming bytes when there is no such frame (saturating at 2^56 - 1);
//   closed  a CLOSE came before (or the incoming state has CLOSED).
// A run of frames is summarised by WsProtoSum; ws_proto_comb is associative (a "last writer", a
// sum that a FIN restarts, a min, and a fence: everything after a run's first CLOSE is dead and
// adds nothing), so a connection may be cut into tiles anywhere and folded in any grouping. The
// state word is itself a summary (ws_proto_sum_state), and every frame's code is
// ws_proto_code(fold of everything before it, the frame). Frames in error still count: the
// state is defined over the live frames, whether or not they are in error.
//
// CLOSE codes: 1000-1003 and 1007-1011 are RFC 6455 7.4.1's; 1012-1014 (service restart, try
// again later, bad gateway) are accepted because IANA has registered them since; 1004-1006 and
// 1015 are reserved and must not appear on the wire; 3000-4999 belong to libraries and
// applications. The CLOSE reason's UTF-8 is the text validator's job (ws_utf8.h).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define WS_PROTO_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define WS_PROTO_FN static inline
#endif

// frame codes (include/wsframe_amd_proto.h: WEBSOCKET_PROTO_*)
#define WS_PROTO_OK 0u
#define WS_PROTO_ERR_RSV 1u
#define WS_PROTO_ERR_OPCODE 2u
#define WS_PROTO_ERR_MASK 3u
#define WS_PROTO_ERR_CTL_FRAGMENTED 4u
#define WS_PROTO_ERR_CTL_LENGTH 5u
#define WS_PROTO_ERR_CLOSE_LENGTH 6u
#define WS_PROTO_ERR_CLOSE_CODE 7u
#define WS_PROTO_ERR_CONT_UNEXPECTED 8u
#define WS_PROTO_ERR_DATA_INTERLEAVED 9u
#define WS_PROTO_ERR_TOO_BIG 10u
#define WS_PROTO_AFTER_CLOSE 0x80u
#define WS_PROTO_NOT_CONSUMED 0x81u
// flags
#define WS_PROTO_F_EXPECT_MASKED 1u
#define WS_PROTO_F_EXPECT_UNMASKED 2u
#define WS_PROTO_F_WIRE_MASKED 4u
#define WS_PROTO_F_ALL 7u
// the state word
#define WS_PROTO_ST_OPEN (1ull << 63)
#define WS_PROTO_ST_CLOSED (1ull << 62)
#define WS_PROTO_BYTES_MAX ((1ull << 56) - 1)
#define WS_PROTO_NONE 0xFFFFFFFFu

// the call's rule parameters
struct WsProtoCfg {
    uint32_t flags, rsv_allowed;
    uint64_t max_message_size;
};

// one consumed frame: its first header byte (the RSV bits), the descriptor's fields and, for a
// CLOSE with 2..125 body bytes, the unmasked status code (else unused)
struct WsProtoFrame {
    uint32_t b0, type, fin, masked, close_code;
    uint64_t datalen;
};

// Summary of a run of consumed frames. `close` is the index (the caller's numbering) of the
// run's first CLOSE; the data fields cover the frames up to it only.
#define WS_PROTO_S_DATA 1u      // the run has a live data frame
#define WS_PROTO_S_LASTFIN 2u   // ... and the last one has FIN
#define WS_PROTO_S_HASFIN 4u    // ... and some one has FIN
#define WS_PROTO_S_HEAD 8u      // (segmented scans: the run starts a new connection; ws_proto_comb_seg)
struct WsProtoSum {
    uint32_t bits;
    uint32_t close;     // WS_PROTO_NONE: no CLOSE in the run
    uint64_t bytes;     // datalen sum of the live data frames after the last one with FIN (all of them: no HASFIN)
};

WS_PROTO_FN uint64_t ws_proto_sat_add(uint64_t a, uint64_t b) {   // a, b <= WS_PROTO_BYTES_MAX
    return a + b > WS_PROTO_BYTES_MAX ? WS_PROTO_BYTES_MAX : a + b;
}
WS_PROTO_FN uint64_t ws_proto_clamp(uint64_t v) { return v > WS_PROTO_BYTES_MAX ? WS_PROTO_BYTES_MAX : v; }

WS_PROTO_FN WsProtoSum ws_proto_sum_none() { return WsProtoSum{0u, WS_PROTO_NONE, 0ull}; }

// the summary of one consumed frame with index k
WS_PROTO_FN WsProtoSum ws_proto_sum_frame(uint32_t type, uint32_t fin, uint64_t datalen, uint32_t k) {
    WsProtoSum s = ws_proto_sum_none();
    if (type == 8u) s.close = k;
    if (!(type & 8u)) {
        s.bits = WS_PROTO_S_DATA | (fin ? WS_PROTO_S_LASTFIN | WS_PROTO_S_HASFIN : 0u);
        s.bytes = fin ? 0ull : ws_proto_clamp(datalen);
    }
    return s;
}

// a then b
WS_PROTO_FN WsProtoSum ws_proto_comb(WsProtoSum a, WsProtoSum b) {
    if (a.close != WS_PROTO_NONE || !(b.bits & WS_PROTO_S_DATA)) {   // b is dead, or adds no data frame
        if (a.close == WS_PROTO_NONE) a.close = b.close;
        return a;
    }
    WsProtoSum r;
    r.bits = WS_PROTO_S_DATA | (b.bits & WS_PROTO_S_LASTFIN) | ((a.bits | b.bits) & WS_PROTO_S_HASFIN);
    r.close = b.close;
    r.bytes = (b.bits & WS_PROTO_S_HASFIN) ? b.bytes : ws_proto_sat_add(a.bytes, b.bytes);
    return r;
}

// the same for a scan over several connections laid end to end: a run that starts a connection
// (HEAD) forgets what came before it
WS_PROTO_FN WsProtoSum ws_proto_comb_seg(WsProtoSum a, WsProtoSum b) {
    if (b.bits & WS_PROTO_S_HEAD) return b;
    WsProtoSum r = ws_proto_comb(a, b);
    r.bits = (r.bits & ~WS_PROTO_S_HEAD) | (a.bits & WS_PROTO_S_HEAD);
    return r;
}

// The incoming state as the summary of everything before the batch. CLOSED is not part of it:
// a closed connection has no live frame at all (ws_proto_code's `closed`).
WS_PROTO_FN WsProtoSum ws_proto_sum_state(uint64_t st) {
    WsProtoSum s;
    s.bits = WS_PROTO_S_DATA | ((st & WS_PROTO_ST_OPEN) ? 0u : WS_PROTO_S_LASTFIN);
    s.close = WS_PROTO_NONE;
    s.bytes = st & WS_PROTO_BYTES_MAX;
    return s;
}

// The state after a batch whose consumed frames fold to `all` (without the incoming state).
WS_PROTO_FN uint64_t ws_proto_state_out(uint64_t st_in, WsProtoSum all) {
    st_in &= WS_PROTO_ST_OPEN | WS_PROTO_ST_CLOSED | WS_PROTO_BYTES_MAX;
    if (st_in & WS_PROTO_ST_CLOSED) return st_in;                 // no live frame
    uint64_t out = st_in;
    if (all.bits & WS_PROTO_S_DATA) {
        const WsProtoSum t = ws_proto_comb(ws_proto_sum_state(st_in), all);
        out = (t.bits & WS_PROTO_S_LASTFIN) ? 0ull : WS_PROTO_ST_OPEN | t.bytes;
    }
    if (all.close != WS_PROTO_NONE) out |= WS_PROTO_ST_CLOSED;
    return out;
}

WS_PROTO_FN uint32_t ws_proto_close_code_ok(uint32_t c) {
    return (uint32_t)((c >= 1000u && c <= 1003u) || (c >= 1007u && c <= 1014u) || (c >= 3000u && c <= 4999u));
}

// Code of the consumed frame f after `before` = ws_proto_comb(ws_proto_sum_state(state in),
// fold of the batch's consumed frames before f); `closed`: the incoming state has CLOSED.
WS_PROTO_FN uint32_t ws_proto_code(WsProtoSum before, uint32_t closed, const WsProtoFrame& f, const WsProtoCfg& c) {
    if (closed || before.close != WS_PROTO_NONE) return WS_PROTO_AFTER_CLOSE;
    if (f.b0 & 0x70u & ~c.rsv_allowed) return WS_PROTO_ERR_RSV;
    if ((f.type >= 3u && f.type <= 7u) || f.type >= 11u) return WS_PROTO_ERR_OPCODE;
    if (((c.flags & WS_PROTO_F_EXPECT_MASKED) && !f.masked) || ((c.flags & WS_PROTO_F_EXPECT_UNMASKED) && f.masked))
        return WS_PROTO_ERR_MASK;
    if (f.type & 8u) {
        if (!f.fin) return WS_PROTO_ERR_CTL_FRAGMENTED;
        if (f.datalen > 125u) return WS_PROTO_ERR_CTL_LENGTH;
        if (f.type == 8u && f.datalen == 1u) return WS_PROTO_ERR_CLOSE_LENGTH;
        if (f.type == 8u && f.datalen >= 2u && !ws_proto_close_code_ok(f.close_code)) return WS_PROTO_ERR_CLOSE_CODE;
        return WS_PROTO_OK;
    }
    const uint32_t open = !(before.bits & WS_PROTO_S_LASTFIN);
    if (f.type == 0u && !open) return WS_PROTO_ERR_CONT_UNEXPECTED;
    if (f.type != 0u && open) return WS_PROTO_ERR_DATA_INTERLEAVED;
    if (c.max_message_size && ws_proto_sat_add(before.bytes, ws_proto_clamp(f.datalen)) > c.max_message_size)
        return WS_PROTO_ERR_TOO_BIG;
    return WS_PROTO_OK;
}

// does the rule read f's CLOSE status code?
WS_PROTO_FN uint32_t ws_proto_reads_close_code(uint32_t type, uint64_t datalen) {
    return (uint32_t)(type == 8u && datalen >= 2u && datalen <= 125u);
}

// 1002 (protocol error), 1009 (message too big), 0: the close status an error code asks for
WS_PROTO_FN uint32_t ws_proto_close_status(uint32_t code) {
    return code == WS_PROTO_ERR_TOO_BIG ? 1009u : (code >= 1u && code <= 10u ? 1002u : 0u);
}

// One frame at a time: f's code, and the state moved past it.
WS_PROTO_FN uint32_t ws_proto_step(uint64_t* state, const WsProtoFrame& f, const WsProtoCfg& c) {
    const uint64_t st = *state;
    const uint32_t code = ws_proto_code(ws_proto_sum_state(st), (uint32_t)((st & WS_PROTO_ST_CLOSED) != 0), f, c);
    *state = ws_proto_state_out(st, ws_proto_sum_frame(f.type, f.fin, f.datalen, 0u));
    return code;
}
