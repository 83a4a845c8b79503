// ws_send.h — the rule of the batch message send (include/wsframe_amd_send.h), defined once: how
// a message is cut into frames, its wire length in closed form, the byte at any wire position of
// a message, what a message slot contributes to its connection and how two such summaries
// combine, the record the kernels keep per message, and where the kernels' scratch lies.
// Plain C++ — no HIP header, no AMDGPU builtin — so the kernels (ws_send.hip), the host entry
// point (websocketframeSendHost) and a host driver (tests/c/send_host.cpp,
// tests/test_send_host.py) build the same text and cannot drift apart.
//
// The rule restates what a stream channel of the reference does with one send: its sharding loop
// (net_reactor.c:871-945, with write_fragment_with_hdr = 1 and on_hdrsize = the frame header
// length, as NetChannelEx_init sets a websocket channel up) cuts the body into packets, and the
// on_pre_send glue writes every packet's header with websocketframeEncode(hdr, fragment_eof, the
// previous packet's fragment_eof, type, bodylen) (websocketframe.c:176-202):
//   H(n)  = websocketframeEncodeHeadLength(n): 2 (n < 126), 4 (n <= 0xFFFF), else 10;
//           in the client role 4 more, for the key bytes;
//   shard = F - H(F), F the channel's write_fragment_size (u32). The header length is taken at F,
//           not at the shard — the reference's quirk: F = 125 gives 123, F = 126 gives 122,
//           F = 65536 gives 65526. F <= H(F): the reference returns NULL, here
//           WEBSOCKET_SEND_ERR_FRAGMENT_SIZE (raised, as there, by a message with a body: an empty
//           message never looks at the shard);
//   L = 0 one frame (FIN, T, empty body);
//   L > 0 n = ceil(L / shard) frames, frame j carrying min(shard, L - j * shard) bytes, opcode T
//         for j = 0 and 0 (continuation) after it, FIN on the last one only, each header as long as
//         its own body asks: H(frame's size).
// T is written as given (T & 0x0F): the reference validates nothing. Lengths are u64 here; the
// reference's nbytes is an unsigned int, so the rule equals the reference wherever L < 2^32.
// Client role (a key per message): MASK bit, the 4 key bytes after the length, the body XORed by
// byte position with the frame's key; fragment j's key is ws_send_frag_key(key, j) =
// key ^ (j * 0x9E3779B9) (j's low 32 bits), so the fragments of one message do not share a key.
// RSV1 (the ext entry points of include/wsframe_amd_compress.h, under WS_SEND_F_RSV1 only): an
// entry whose T has WS_SEND_T_RSV1 set carries 0x40 on frame 0's first byte and on no other frame.
// The bit travels in the record's type word (ws_send_rec_type: the opcode, and WS_SEND_REC_RSV1
// for that bit); it changes no length.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/wsframe_amd_send.h"

#ifdef __HIPCC__
#define WS_SEND_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define WS_SEND_FN static inline
#endif

#define WS_SEND_NONE 0xFFFFFFFFu
#define WS_SEND_F_RSV1 1u             // flags of the ext entry points: WEBSOCKET_SEND_FLAG_RSV1
#define WS_SEND_T_RSV1 0x40u          // WebsocketSendMsg_t.type: WEBSOCKET_SEND_TYPE_RSV1
#define WS_SEND_REC_RSV1 0x80000000u  // WsSendRec.type: frame 0 carries RSV1
#define WS_SEND_SRC_MAX (1ull << 56)   // src_len above this is refused: 7 * L (the 3-byte frames of F = 7) stays a u64

// ------------------------------------------------------------------------------------- geometry

WS_SEND_FN uint32_t ws_send_head_len(uint64_t n) { return n < 126u ? 2u : (n <= 0xFFFFu ? 4u : 10u); }
WS_SEND_FN uint32_t ws_send_hdr_len(uint64_t n, uint32_t role) { return ws_send_head_len(n) + (role ? 4u : 0u); }
// the body bytes of a full frame; 0: F is too small to carry a byte
WS_SEND_FN uint32_t ws_send_shard(uint32_t F, uint32_t role) {
    const uint32_t h = ws_send_hdr_len(F, role);
    return F <= h ? 0u : F - h;
}
WS_SEND_FN uint32_t ws_send_frag_key(uint32_t key, uint64_t j) { return key ^ ((uint32_t)j * 0x9E3779B9u); }
// wire bytes of a full frame (shard > 0); at most F, so a u32
WS_SEND_FN uint32_t ws_send_stride(uint32_t shard, uint32_t role) { return ws_send_hdr_len(shard, role) + shard; }

struct WsSendGeo { uint64_t frames, wire; };
// frames and wire bytes of a message of L body bytes (shard > 0 unless L == 0)
WS_SEND_FN WsSendGeo ws_send_geo(uint64_t L, uint32_t shard, uint32_t role) {
    WsSendGeo g;
    if (L == 0) {
        g.frames = 1;
        g.wire = ws_send_hdr_len(0, role);
        return g;
    }
    g.frames = (L - 1) / shard + 1;
    const uint64_t last = L - (g.frames - 1) * shard;
    g.wire = (g.frames - 1) * (uint64_t)ws_send_stride(shard, role) + ws_send_hdr_len(last, role) + last;
    return g;
}

// What the kernels keep per message slot. 48 bytes. A slot that sends nothing (a SKIP entry, a
// slot past the connection's count, any slot of a failed connection) has wire == 0 and keeps its
// place: tx_off never decreases with the slot index.
struct WsSendRec {
    uint64_t tx_off;              // the message's first wire byte in d_tx
    uint64_t src_off, len;        // its body in d_src
    uint64_t wire;                // its wire bytes
    uint32_t shard, key;          // the connection's shard; the message's key (client role)
    uint32_t type, role;          // opcode of the first frame (| WS_SEND_REC_RSV1); 1: client role
};
// the record's type word of an entry's T under the call's flags
WS_SEND_FN uint32_t ws_send_rec_type(uint32_t T, uint32_t flags) {
    return (T & 0x0Fu) | ((flags & WS_SEND_F_RSV1) && (T & WS_SEND_T_RSV1) ? WS_SEND_REC_RSV1 : 0u);
}

// Where wire position p < r.wire of the message lies: its frame, the frame's first body byte in
// the message, the position inside the frame, the frame's body bytes and H of them. One 64-bit
// division when p >= 2^32, else a 32-bit one (the stride is a u32).
struct WsSendLoc { uint64_t j, body0; uint32_t q, flen, hl, pad; };
WS_SEND_FN WsSendLoc ws_send_locate(const WsSendRec& r, uint64_t p) {
    WsSendLoc f = {0ull, 0ull, (uint32_t)p, 0u, 2u, 0u};
    if (r.len) {
        const uint32_t stride = ws_send_stride(r.shard, r.role);
        f.j = (p >> 32) ? p / stride : (uint64_t)((uint32_t)p / stride);
        f.q = (uint32_t)(p - f.j * stride);
        f.body0 = f.j * r.shard;
        const uint64_t left = r.len - f.body0;
        f.flen = left < r.shard ? (uint32_t)left : r.shard;
        f.hl = ws_send_head_len(f.flen);
    }
    return f;
}
// byte w of frame f of the message: header, key or body
WS_SEND_FN unsigned char ws_send_frame_byte(const WsSendRec& r, const unsigned char* src, const WsSendLoc& f, uint32_t w) {
    const uint32_t hl = f.hl, fk = ws_send_frag_key(r.key, f.j);
    if (w == 0u)
        return (unsigned char)((f.body0 + f.flen == r.len ? 0x80u : 0u) | (f.j == 0 ? (r.type & 0x0Fu) | (r.type >> 31 << 6) : 0u));
    if (w < hl) {
        const uint32_t m = r.role ? 0x80u : 0u;
        if (w == 1u) return (unsigned char)((hl == 2u ? f.flen : (hl == 4u ? 126u : 127u)) | m);
        return (unsigned char)((uint64_t)f.flen >> (8u * (hl - 1u - w)));   // big-endian, 16 or 64 bits
    }
    if (r.role && w < hl + 4u) return (unsigned char)(fk >> (8u * (w - hl)));
    const uint32_t k = w - hl - (r.role ? 4u : 0u);
    uint32_t v = src[r.src_off + f.body0 + k];
    if (r.role) v ^= fk >> (8u * (k & 3u));
    return (unsigned char)v;
}
// The byte at wire position p < r.wire of the message (src: d_src).
WS_SEND_FN unsigned char ws_send_byte(const WsSendRec& r, const unsigned char* src, uint64_t p) {
    const WsSendLoc f = ws_send_locate(r, p);
    return ws_send_frame_byte(r, src, f, f.q);
}

// ------------------------------------------------------------------------------------ run summary

#define WS_SEND_S_HEAD 1u         // (segmented scans: the run starts a new connection; ws_send_comb_seg)
struct WsSendSum {                // 32 bytes
    uint32_t bits;
    uint32_t first_bad;           // index of the run's first failing message, else WS_SEND_NONE
    uint32_t status;              // ... and its WEBSOCKET_SEND_ERR_*
    uint32_t nmsg;                // messages that send something
    uint64_t bytes, frames;       // their wire bytes and frames
};

WS_SEND_FN WsSendSum ws_send_sum_none() { return WsSendSum{0u, WS_SEND_NONE, 0u, 0u, 0ull, 0ull}; }

// the summary of message i of a connection with fragment size F
WS_SEND_FN WsSendSum ws_send_sum_msg(const WebsocketSendMsg_t& m, uint32_t i, uint64_t src_len, uint32_t F, uint32_t role) {
    WsSendSum s = ws_send_sum_none();
    if (m.type == WEBSOCKET_SEND_SKIP) return s;
    const uint32_t shard = ws_send_shard(F, role);
    if (m.len > src_len || m.src_off > src_len - m.len) {
        s.first_bad = i;
        s.status = WEBSOCKET_SEND_ERR_RANGE;
    } else if (m.len && !shard) {
        s.first_bad = i;
        s.status = WEBSOCKET_SEND_ERR_FRAGMENT_SIZE;
    } else {
        const WsSendGeo g = ws_send_geo(m.len, shard, role);
        s.nmsg = 1u;
        s.bytes = g.wire;
        s.frames = g.frames;
    }
    return s;
}

// a then b. Sums and a "first": associative. The sums of a failed run are carried along and
// dropped where the connection's result is formed (ws_send_result).
WS_SEND_FN WsSendSum ws_send_comb(WsSendSum a, WsSendSum b) {
    if (a.first_bad == WS_SEND_NONE) {
        a.first_bad = b.first_bad;
        a.status = b.status;
    }
    a.nmsg += b.nmsg;
    a.bytes += b.bytes;
    a.frames += b.frames;
    return a;
}
// the same for a scan over several connections laid end to end
WS_SEND_FN WsSendSum ws_send_comb_seg(WsSendSum a, WsSendSum b) {
    if (b.bits & WS_SEND_S_HEAD) return b;
    WsSendSum r = ws_send_comb(a, b);
    r.bits = a.bits & WS_SEND_S_HEAD;
    return r;
}

// a connection's result from the fold of all its slots: all or nothing
WS_SEND_FN WebsocketSendResult_t ws_send_result(const WsSendSum& all) {
    WebsocketSendResult_t r;
    const int ok = all.first_bad == WS_SEND_NONE;
    r.tx_len = ok ? all.bytes : 0ull;
    r.n_frames = ok ? all.frames : 0ull;
    r.n_msgs = ok ? all.nmsg : 0u;
    r.status = ok ? WEBSOCKET_SEND_OK : all.status;
    r.first_bad = all.first_bad;
    r.reserved = 0u;
    return r;
}

// --------------------------------------------------------------------- one connection, sequentially

// The whole rule for one connection (the host entry point; the kernels do the same in passes):
// msg[0, nmsg), keys (NULL: server role) one per message slot, tx[0, cap) the wire bytes,
// msg_tx_off (may be NULL) every message's first wire byte. Returns the full length.
// flags: 0, or WS_SEND_F_RSV1 (the ext entry point).
WS_SEND_FN uint64_t ws_send_connection_ext(const unsigned char* src, uint64_t src_len, const WebsocketSendMsg_t* msg,
                                           uint32_t nmsg, uint32_t F, const uint32_t* keys, uint32_t flags, unsigned char* tx,
                                           uint64_t cap, uint64_t* msg_tx_off, WebsocketSendResult_t* out) {
    const uint32_t role = keys ? 1u : 0u, shard = ws_send_shard(F, role);
    WsSendSum all = ws_send_sum_none();
    for (uint32_t i = 0; i < nmsg; ++i) all = ws_send_comb(all, ws_send_sum_msg(msg[i], i, src_len, F, role));
    *out = ws_send_result(all);
    uint64_t off = 0;
    for (uint32_t i = 0; i < nmsg; ++i) {
        if (msg_tx_off) msg_tx_off[i] = off;
        if (out->status != WEBSOCKET_SEND_OK || msg[i].type == WEBSOCKET_SEND_SKIP) continue;
        WsSendRec r = {off, msg[i].src_off, msg[i].len, ws_send_geo(msg[i].len, shard, role).wire, shard,
                       keys ? keys[i] : 0u, ws_send_rec_type(msg[i].type, flags), role};
        for (uint64_t p = 0; p < r.wire && off + p < cap; ++p) tx[off + p] = ws_send_byte(r, src, p);
        off += r.wire;
    }
    return off;
}
WS_SEND_FN uint64_t ws_send_connection(const unsigned char* src, uint64_t src_len, const WebsocketSendMsg_t* msg,
                                       uint32_t nmsg, uint32_t F, const uint32_t* keys, unsigned char* tx, uint64_t cap,
                                       uint64_t* msg_tx_off, WebsocketSendResult_t* out) {
    return ws_send_connection_ext(src, src_len, msg, nmsg, F, keys, 0u, tx, cap, msg_tx_off, out);
}

// ------------------------------------------------------------------------------ kernel scratch

// The workspace, every part 16-B aligned: [head: 16 B][bo64: wire byte offsets of the blocks of 256
// connections, nb + 1 u64][loc: a connection's offset inside its block, nb * 256 u64][tail: nseg
// summaries, a connection's slots inside its last tile][agg: one summary per tile of 256 slots]
// [rec: one record per slot][ptr: for every 16 KiB piece of d_tx (counted from the 16-B block
// d_tx's base lies in) below the capacity, the slot whose message holds the piece's first byte]
#define WS_SEND_T 256u
#define WS_SEND_PIECE_SHIFT 14
struct WsSendLayout { size_t bo64, loc, tail, agg, rec, ptr, bytes; uint32_t nb, ntiles; uint64_t npieces; };
static inline WsSendLayout ws_send_layout(uint32_t nseg, uint32_t max_msgs, uint64_t tx_capacity) {
    WsSendLayout L;
    const uint64_t nslots = (uint64_t)nseg * max_msgs;
    L.nb = (nseg + WS_SEND_T - 1) / WS_SEND_T;
    L.ntiles = (uint32_t)((nslots + WS_SEND_T - 1) / WS_SEND_T);
    L.npieces = tx_capacity ? ((tx_capacity + 15) >> WS_SEND_PIECE_SHIFT) + 1 : 0;   // (+ 15: the base's phase)
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    L.bo64 = 16;
    L.loc = L.bo64 + up16(((size_t)L.nb + 1) * 8);
    L.tail = L.loc + (size_t)L.nb * WS_SEND_T * 8;
    L.agg = L.tail + (size_t)nseg * sizeof(WsSendSum);
    L.rec = L.agg + (size_t)L.ntiles * sizeof(WsSendSum);
    L.ptr = L.rec + (size_t)nslots * sizeof(WsSendRec);
    L.bytes = L.ptr + up16((size_t)L.npieces * 4);
    return L;
}
// pieces that hold a byte of [0, limit) of a d_tx whose base lies lead (< 16) bytes into its 16-B block
WS_SEND_FN uint64_t ws_send_pieces(uint64_t limit, uint32_t lead) {
    return limit ? ((limit + lead - 1) >> WS_SEND_PIECE_SHIFT) + 1 : 0;
}
