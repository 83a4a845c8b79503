// ws_reply.h — the rule of the control replies (RFC 6455 5.5.1-5.5.3, 7.1.7;
// include/wsframe_amd_reply.h), defined once: what a frame contributes to its connection's reply,
// the summary of a run of frames and how two summaries combine, what a segment sends given the
// summary of all its frames, the bytes of a reply frame, and where the kernels' scratch lies.
// Plain C++ — no HIP header, no AMDGPU builtin — so the kernels (ws_reply.hip), the host entry
// point (websocketframeControlRepliesHost) and a host driver (tests/c/reply_host.cpp,
// tests/test_reply_host.py) build the same text and cannot drift apart.
//
// Scan form. A PONG's place in its segment's reply is the sum of the PONG bytes before it, and
// PONGs stop at end = min(first_bad, first CLOSE). first_bad is known per segment before any
// frame is looked at, so a frame at or past it simply contributes nothing; the first CLOSE is
// found by the scan itself, with ws_proto.h's fence: everything after a run's first CLOSE is dead
// and adds nothing. WsReplySum holds a run's PONG count and bytes up to its first CLOSE, that
// CLOSE's index and the last answerable ping (index and PONG length, for LAST_PING_ONLY);
// ws_reply_comb is associative (two sums, a "first", a "last writer" and the fence), so a
// connection may be cut into tiles anywhere and folded in any grouping.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/wsframe_amd_reply.h"

#ifdef __HIPCC__
#define WS_REPLY_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define WS_REPLY_FN static inline
#endif

#define WS_REPLY_F_ALL (WEBSOCKET_REPLY_WIRE_MASKED | WEBSOCKET_REPLY_LAST_PING_ONLY)
#define WS_REPLY_NONE 0xFFFFFFFFu
#define WS_REPLY_PONG_B0 0x8Au    // what websocketframeEncode(head, 1, 1, 10, T) writes first
#define WS_REPLY_CLOSE_B0 0x88u   // ... and websocketframeEncode(head, 1, 1, 8, T)

// ------------------------------------------------------------------------- per-frame contribution

// does a consumed frame before `end` get a PONG?
WS_REPLY_FN uint32_t ws_reply_answerable(uint32_t type, uint32_t fin, uint64_t datalen) {
    return (uint32_t)(type == 9u && fin != 0u && datalen <= 125u);
}
// bytes of a reply frame with `body` (<= 125) body bytes: two header bytes, the key when masked
WS_REPLY_FN uint32_t ws_reply_frame_len(uint32_t body, uint32_t keyed) { return 2u + (keyed ? 4u : 0u) + body; }

// ------------------------------------------------------------------------------------ run summary

#define WS_REPLY_S_HEAD 1u        // (segmented scans: the run starts a new connection; ws_reply_comb_seg)
struct WsReplySum {               // 32 bytes; the pong fields cover the frames before `close` only
    uint32_t bits;
    uint32_t close;               // index (the caller's numbering) of the run's first CLOSE, else WS_REPLY_NONE
    uint32_t npong;               // answerable pings
    uint32_t last;                // the last of them, else WS_REPLY_NONE
    uint64_t bytes;               // bytes of their PONGs
    uint32_t last_bytes;          // bytes of the last one's PONG
    uint32_t pad;
};

WS_REPLY_FN WsReplySum ws_reply_sum_none() { return WsReplySum{0u, WS_REPLY_NONE, 0u, WS_REPLY_NONE, 0ull, 0u, 0u}; }

// the summary of one consumed frame with index k; live: k < first_bad
WS_REPLY_FN WsReplySum ws_reply_sum_frame(uint32_t type, uint32_t fin, uint64_t datalen, uint32_t k, uint32_t live,
                                          uint32_t keyed) {
    WsReplySum s = ws_reply_sum_none();
    if (type == 8u) s.close = k;
    if (live && ws_reply_answerable(type, fin, datalen)) {
        s.npong = 1u;
        s.last = k;
        s.bytes = s.last_bytes = ws_reply_frame_len((uint32_t)datalen, keyed);
    }
    return s;
}

// a then b
WS_REPLY_FN WsReplySum ws_reply_comb(WsReplySum a, WsReplySum b) {
    if (a.close != WS_REPLY_NONE) return a;            // b is dead
    a.close = b.close;
    a.npong += b.npong;
    a.bytes += b.bytes;
    if (b.last != WS_REPLY_NONE) {
        a.last = b.last;
        a.last_bytes = b.last_bytes;
    }
    return a;
}

// the same for a scan over several connections laid end to end: a run that starts a connection
// (HEAD) forgets what came before it
WS_REPLY_FN WsReplySum ws_reply_comb_seg(WsReplySum a, WsReplySum b) {
    if (b.bits & WS_REPLY_S_HEAD) return b;
    WsReplySum r = ws_reply_comb(a, b);
    r.bits = a.bits & WS_REPLY_S_HEAD;
    return r;
}

// ------------------------------------------------------------------------- what a segment sends

// which CLOSE ends the reply of a segment whose frames fold to `all`
WS_REPLY_FN uint32_t ws_reply_close_kind(const WsReplySum& all, uint32_t first_bad, uint32_t fail_status) {
    if (first_bad != WS_REPLY_NONE && first_bad <= all.close) return WEBSOCKET_REPLY_CLOSE_PROTOCOL;
    if (fail_status) return WEBSOCKET_REPLY_CLOSE_CALLER;
    return all.close != WS_REPLY_NONE ? WEBSOCKET_REPLY_CLOSE_ECHO : WEBSOCKET_REPLY_CLOSE_NONE;
}

struct WsReplySeg {
    uint32_t end;          // pings at k >= end are silent
    uint32_t only;         // LAST_PING_ONLY: the one ping answered (WS_REPLY_NONE: none); else unused
    uint32_t npong;
    uint32_t close_kind, close_status, close_len;   // close_len: bytes of the CLOSE frame, 0 = none
    uint64_t pong_bytes;   // the CLOSE's offset in the segment's reply
};

// `all`: the fold of the segment's consumed frames; state_in: the carry; kind: ws_reply_close_kind;
// status: what that kind sends (PROTOCOL: close_status, CALLER: fail_status, ECHO: the echoed
// code); body: the CLOSE's body bytes, 2 except for an ECHO of a CLOSE shorter than 2
WS_REPLY_FN WsReplySeg ws_reply_seg(const WsReplySum& all, uint32_t first_bad, uint32_t state_in, uint32_t flags,
                                    uint32_t keyed, uint32_t kind, uint32_t status, uint32_t body) {
    WsReplySeg g = {0u, WS_REPLY_NONE, 0u, 0u, 0u, 0u, 0ull};
    if (state_in & WEBSOCKET_REPLY_ST_CLOSE_SENT) return g;
    g.end = first_bad < all.close ? first_bad : all.close;
    if (flags & WEBSOCKET_REPLY_LAST_PING_ONLY) {
        g.only = all.last;
        g.npong = all.last != WS_REPLY_NONE ? 1u : 0u;
        g.pong_bytes = all.last != WS_REPLY_NONE ? all.last_bytes : 0u;
    } else {
        g.npong = all.npong;
        g.pong_bytes = all.bytes;
    }
    g.close_kind = kind;
    if (kind != WEBSOCKET_REPLY_CLOSE_NONE) {
        g.close_status = body ? status & 0xFFFFu : 0u;
        g.close_len = ws_reply_frame_len(body, keyed);
    }
    return g;
}

// is frame k (consumed, with the segment's plan g) answered?
WS_REPLY_FN uint32_t ws_reply_answers(const WsReplySeg& g, uint32_t flags, uint32_t k, uint32_t type, uint32_t fin,
                                      uint64_t datalen) {
    if (k >= g.end || !ws_reply_answerable(type, fin, datalen)) return 0u;
    return (uint32_t)(!(flags & WEBSOCKET_REPLY_LAST_PING_ONLY) || k == g.only);
}

// ----------------------------------------------------------------------------------- frame writer

// One reply frame: first byte, body length, the reply key (keyed: the MASK bit and 4 key bytes, as
// ws_encode.hip adds them; key byte i = key >> 8 * i), and its body: src[i], XORed with
// unmask[i & 3] where unmask is set (a body still masked on the wire), or, where src is NULL, the
// big-endian bytes of `status`.
struct WsReplyFrame {
    uint32_t b0, len, keyed, key, status;
    const unsigned char* src;
    const unsigned char* unmask;
};
// byte j < ws_reply_frame_len(f.len, f.keyed) of the frame
WS_REPLY_FN unsigned char ws_reply_byte(const WsReplyFrame& f, uint32_t j) {
    const uint32_t hdr = f.keyed ? 6u : 2u;
    if (j == 0u) return (unsigned char)f.b0;
    if (j == 1u) return (unsigned char)(f.len | (f.keyed ? 0x80u : 0u));
    if (j < hdr) return (unsigned char)(f.key >> (8u * (j - 2u)));
    const uint32_t i = j - hdr;
    uint32_t v = f.src ? f.src[i] : (f.status >> (8u * (1u - (i & 1u)))) & 0xFFu;
    if (f.src && f.unmask) v ^= f.unmask[i & 3u];
    if (f.keyed) v ^= f.key >> (8u * (i & 3u));
    return (unsigned char)v;
}
// the PONG answering a ping whose body lies at buf + data_off (an empty body has no address:
// WEBSOCKET_DATA_OFF_NULL); wire_masked: the call's WIRE_MASKED flag and the descriptor's
// `masked`: the key is the four bytes before the body
WS_REPLY_FN WsReplyFrame ws_reply_pong(const unsigned char* buf, uint64_t data_off, uint32_t datalen, uint32_t wire_masked,
                                       uint32_t keyed, uint32_t key) {
    const unsigned char* const body = datalen ? buf + data_off : buf;
    return WsReplyFrame{WS_REPLY_PONG_B0, datalen, keyed, key, 0u, body, wire_masked && datalen ? body - 4 : nullptr};
}
WS_REPLY_FN WsReplyFrame ws_reply_close(uint32_t status, uint32_t body, uint32_t keyed, uint32_t key) {
    return WsReplyFrame{WS_REPLY_CLOSE_B0, body, keyed, key, status, nullptr, nullptr};
}
// write the frame at tx + off, never at or past cap
WS_REPLY_FN void ws_reply_write(const WsReplyFrame& f, unsigned char* tx, uint64_t off, uint64_t cap) {
    const uint32_t n = ws_reply_frame_len(f.len, f.keyed);
    for (uint32_t j = 0; j < n && off + j < cap; ++j) tx[off + j] = ws_reply_byte(f, j);
}

// the status an ECHO sends: the first two unmasked body bytes of the CLOSE at `body`
WS_REPLY_FN uint32_t ws_reply_echo_status(const unsigned char* body, uint32_t wire_masked) {
    uint32_t c0 = body[0], c1 = body[1];
    if (wire_masked) {
        c0 ^= body[-4];
        c1 ^= body[-3];
    }
    return c0 << 8 | c1;
}

// --------------------------------------------------------------------- one segment, sequentially

WS_REPLY_FN uint32_t ws_reply_consumed(const WebsocketFrameDesc_t& d, uint64_t seg_end) {
    return (uint32_t)(d.ret > 0 && d.frame_off + (uint64_t)d.ret <= seg_end);
}

// The whole rule for one segment (the host entry point; the kernels do the same in passes).
// Returns the reply's full length.
WS_REPLY_FN uint64_t ws_reply_segment(const unsigned char* buf, uint64_t seg_off, const WebsocketFrameDesc_t* desc,
                                      const WebsocketSegResult_t* res, uint32_t max_frames, uint32_t flags,
                                      const WebsocketProtoResult_t* pr, uint32_t fail_status, const uint32_t* keys,
                                      uint32_t* state, unsigned char* tx, uint64_t cap, WebsocketReplyResult_t* out) {
    const uint32_t n = res->n_frames < max_frames ? res->n_frames : max_frames, keyed = keys ? 1u : 0u;
    const uint32_t first_bad = pr ? pr->first_bad : WS_REPLY_NONE;
    const uint32_t wm = flags & WEBSOCKET_REPLY_WIRE_MASKED;
    const uint64_t seg_end = seg_off + res->consumed;
    WsReplySum all = ws_reply_sum_none();
    for (uint32_t k = 0; k < n; ++k)
        if (ws_reply_consumed(desc[k], seg_end))
            all = ws_reply_comb(all, ws_reply_sum_frame(desc[k].type, desc[k].is_fin, desc[k].datalen, k,
                                                        (uint32_t)(k < first_bad), keyed));
    const uint32_t kind = ws_reply_close_kind(all, first_bad, fail_status);
    uint32_t status = 0, body = 2;
    if (kind == WEBSOCKET_REPLY_CLOSE_PROTOCOL) status = pr->close_status;
    else if (kind == WEBSOCKET_REPLY_CLOSE_CALLER) status = fail_status;
    else if (kind == WEBSOCKET_REPLY_CLOSE_ECHO) {
        const WebsocketFrameDesc_t& c = desc[all.close];
        if (c.datalen >= 2) status = ws_reply_echo_status(buf + c.data_off, wm && c.masked);
        else body = 0;
    }
    const WsReplySeg g = ws_reply_seg(all, first_bad, state ? *state : 0u, flags, keyed, kind, status, body);
    uint64_t off = 0;
    for (uint32_t k = 0; k < g.end && k < n; ++k) {
        const WebsocketFrameDesc_t& d = desc[k];
        if (!ws_reply_consumed(d, seg_end) || !ws_reply_answers(g, flags, k, d.type, d.is_fin, d.datalen)) continue;
        ws_reply_write(ws_reply_pong(buf, d.data_off, (uint32_t)d.datalen, wm && d.masked, keyed, keyed ? keys[k] : 0u), tx,
                       off, cap);
        off += ws_reply_frame_len((uint32_t)d.datalen, keyed);
    }
    if (g.close_len) {
        ws_reply_write(ws_reply_close(g.close_status, g.close_len - (keyed ? 6u : 2u), keyed, keyed ? keys[max_frames] : 0u),
                       tx, off, cap);
        if (state) *state |= WEBSOCKET_REPLY_ST_CLOSE_SENT;
    }
    out->n_pong = g.npong;
    out->close_kind = g.close_kind;
    out->close_status = g.close_status;
    out->tx_len = (uint32_t)(g.pong_bytes + g.close_len);
    return g.pong_bytes + g.close_len;
}

// ------------------------------------------------------------------------------ kernel scratch

// What ws_reply.hip keeps per segment between its passes: the segment's offset among the 256
// segments of its block, its PONG bytes (the CLOSE's offset), and what its frames need to know.
struct WsReplyRec {               // 32 bytes
    uint64_t loc_off, pong_bytes;
    uint32_t end, only;
    uint32_t close;               // 0: none; else close_len | close_status << 16
    uint32_t pad;
};

// The workspace, every part 16-B aligned: [head: 16 B][bo: frame offsets of the blocks of 256
// segments, nb + 1 u32][loff: a segment's frame offset inside its block, nb * 256 u32][bo64: reply
// byte offsets of the blocks, nb + 1 u64][rec: nseg records][tail: nseg summaries, a segment's
// frames inside its last tile][agg: one summary per tile of 256 frames]
#define WS_REPLY_T 256u
struct WsReplyLayout { size_t bo, loff, bo64, rec, tail, agg, bytes; uint32_t nb, ntmax; };
static inline WsReplyLayout ws_reply_layout(uint32_t nseg, uint32_t max_frames) {
    WsReplyLayout L;
    const uint64_t nslots = (uint64_t)nseg * max_frames;
    L.nb = (nseg + WS_REPLY_T - 1) / WS_REPLY_T;
    L.ntmax = (uint32_t)((nslots + WS_REPLY_T - 1) / WS_REPLY_T);
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    L.bo = 16;
    L.loff = L.bo + up16(((size_t)L.nb + 1) * 4);
    L.bo64 = L.loff + (size_t)L.nb * WS_REPLY_T * 4;
    L.rec = L.bo64 + up16(((size_t)L.nb + 1) * 8);
    L.tail = L.rec + (size_t)nseg * sizeof(WsReplyRec);
    L.agg = L.tail + (size_t)nseg * sizeof(WsReplySum);
    L.bytes = L.agg + (size_t)L.ntmax * sizeof(WsReplySum);
    return L;
}
