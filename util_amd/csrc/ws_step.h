// ws_step.h — one step of the reactor loop (net_reactor.c:515-526 over websocketframe.c:112-165),
// defined once for every walk: the header parse, what a candidate frame means for the loop, the
// header loads, and what a consumed frame leaves behind for the unmask (item, piece pointers,
// descriptor). A walk only chooses which candidates it looks at and how it advances.
//
// The first part (parse, outcome, status packing) is plain C++ — no HIP header, no AMDGPU
// builtin — so a host compiler can build it and a CPU test can hold it against the oracle
// (tests/test_step_host.py). The second part is device code.
#pragma once
#include <stdint.h>

#include "../../include/wsframe_amd.h"

#ifdef __HIPCC__
#define WS_STEP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define WS_STEP_FN static inline
#endif

typedef unsigned long long u64;
typedef unsigned int u32;

// Result of parsing one frame header (websocketframe.c:112-165).
enum { WS_PARSE_INCOMPLETE = 0, WS_PARSE_FRAME = 1, WS_PARSE_WRAP = 2 };
struct WsHdr {
    int kind;      // WS_PARSE_*
    u32 b0, b1;    // header bytes 0 and 1
    u32 hdr;       // 2 + ext + mask
    u32 masked;    // MASK bit
    u32 key;       // little-endian masking key (valid if masked)
    u64 plen;      // payload length
    int ret;       // (int) return value (:164)
};

// h0 = header bytes 0..7, h1 = bytes 8..15 (little-endian), avail = bytes left (fewer than 2:
// incomplete, websocketframe.c:121).
// Mirrors websocketframe.c:121-164 exactly, plus the batch fence: a MASKED frame
// whose u64 length sum wraps and would pass the :149 check is WS_PARSE_WRAP (the
// reference would unmask past the buffer: undefined behaviour).
WS_STEP_FN WsHdr ws_parse(u64 h0, u64 h1, u64 avail) {
    WsHdr r;
    r.b0 = (u32)h0 & 0xFFu;
    r.b1 = (u32)(h0 >> 8) & 0xFFu;
    const u32 p7 = r.b1 & 0x7Fu;                                   // :129
    r.masked = r.b1 >> 7;                                          // :126-127
    const u32 ext = p7 < 126 ? 0u : (p7 == 126 ? 2u : 8u);         // :134-145
    r.hdr = 2u + ext + (r.masked ? 4u : 0u);
    r.kind = WS_PARSE_INCOMPLETE;
    r.key = 0;
    r.plen = 0;
    r.ret = 0;
    if (avail < r.hdr) return r;                                   // :131,136,142
    if (ext == 0) r.plen = p7;
    else if (ext == 2) r.plen = ((h0 >> 16) & 0xFFu) << 8 | ((h0 >> 24) & 0xFFu);   // memReadBE16
    else r.plen = __builtin_bswap64((h0 >> 16) | (h1 << 48));                          // memReadBE64
    const u64 total = (u64)r.hdr + r.plen;                         // u64, may wrap (:149)
    if (avail < total) return r;                                   // :149-150
    if (r.masked && total < r.plen) { r.kind = WS_PARSE_WRAP; return r; }
    r.key = ext == 0 ? (u32)(h0 >> 16) : (ext == 2 ? (u32)(h0 >> 32) : (u32)(h1 >> 16));
    r.ret = (int)(u32)total;                                       // :164, truncating
    r.kind = WS_PARSE_FRAME;
    return r;
}

// The length of the frame h, 0 unless it is a complete frame with a positive return: the
// stride a walk may speculate with from there.
WS_STEP_FN u32 ws_plain_frame_len(const WsHdr& h) { return h.kind == WS_PARSE_FRAME && h.ret > 0 ? (u32)h.ret : 0u; }

// What the candidate frame at `pos` of a segment of `limit` bytes means for the loop, in the
// reactor's order. `index`: the frames before it; h: its parse (ws_parse with avail = limit - pos;
// not looked at when pos >= limit); g: the stride the walk speculates with; any_len: every
// positive length continues (a walk that does not speculate on one stride).
//   0 consumed, the chain continues          1 consumed, its length differs from g
//   2 consumed, the walk ends (ret <= 0: a descriptor only for ret < 0)
//   3 not consumed, the walk ends            (4: a walk's own "not in my window", never from here)
// status: the segment's WEBSOCKET_SEG_* if the walk ends at this candidate.
WS_STEP_FN u32 ws_cand_code(u64 pos, u64 limit, u64 index, u32 max_frames, const WsHdr& h, u64 g, bool any_len,
                       int& status) {
    status = WEBSOCKET_SEG_OK;
    if (pos >= limit) return 3;
    if (index >= max_frames) { status = WEBSOCKET_SEG_MAX_FRAMES; return 3; }
    if (h.kind == WS_PARSE_INCOMPLETE) return 3;                   // (fewer than 2 bytes left included, :121)
    if (h.kind == WS_PARSE_WRAP) { status = WEBSOCKET_SEG_ERR_LEN_WRAP; return 3; }
    if (h.ret <= 0) { status = h.ret < 0 ? WEBSOCKET_SEG_ERR_DECODE : WEBSOCKET_SEG_OK; return 2; }
    return any_len || (u64)(u32)h.ret == g ? 0u : 1u;
}

// The statuses ws_cand_code gives are -2..1: two bits hold them (the raw stream's packed stop word).
WS_STEP_FN u32 ws_status_bits(int status) { return (u32)status & 3u; }
WS_STEP_FN int ws_bits_status(u32 bits) { return (int)(bits ^ 2u) - 2; }

// the unmask kernel's unit (ws_piece.hip K2, also behind the raw-stream path): one-shot
// 256-thread blocks over WS_PIECE_U KiB per wave, 2^WS_PIECE_SHIFT bytes per block
// (ws_layout.h counts a workspace's pieces by it)
#ifndef WS_PIECE_U
#define WS_PIECE_U 4
#define WS_PIECE_SHIFT 14                   // 16 KiB = 256 threads * WS_PIECE_U * 16 B
#endif

#ifdef __HIPCC__
// ---------------------------------------------------------------------------------------------
// Device part.
#include <hip/hip_runtime.h>

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// Global-address-space views: hot loops must emit global_load/store, not flat_*
// (flat ops complete out of order, so hipcc drains vmcnt+lgkmcnt before each one
// and every load becomes its own round trip).
#define WS_GLOBAL __attribute__((address_space(1)))
typedef WS_GLOBAL u32x4 gu32x4;
typedef WS_GLOBAL u32 gu32;
typedef WS_GLOBAL u64 gu64;
typedef WS_GLOBAL unsigned char gu8;

template <typename T>
__device__ __forceinline__ WS_GLOBAL T* gptr(const void* p) {
    return reinterpret_cast<WS_GLOBAL T*>(reinterpret_cast<uintptr_t>(p));
}

__device__ __forceinline__ u32 rotl32(u32 x, u32 r) { return r ? (x << r) | (x >> (32 - r)) : x; }

// Header bytes [p, p+16) from the 32 bytes x0|x1 loaded at floor16(p), o = p & 15,
// as two little-endian u64 (bytes 0..7, 8..15). Branch-free on purpose: a divergent
// per-lane dword select around these loads produced nondeterministic header reads
// under load on ROCm 7.2.
__device__ __forceinline__ void ws_hdr_from32(const u32x4 x0, const u32x4 x1, u32 o, u64& h0, u64& h1) {
    const u64 w0 = (u64)x0.x | ((u64)x0.y << 32), w1 = (u64)x0.z | ((u64)x0.w << 32);
    const u64 w2 = (u64)x1.x | ((u64)x1.y << 32), w3 = (u64)x1.z | ((u64)x1.w << 32);
    const u32 sh = 8u * (o & 7);
    const bool up = o >= 8;
    const u64 a0 = up ? w1 : w0, a1 = up ? w2 : w1, a2 = up ? w3 : w2;
    h0 = sh ? (a0 >> sh) | (a1 << (64 - sh)) : a0;
    h1 = sh ? (a1 >> sh) | (a2 << (64 - sh)) : a1;
}

// The 16 bytes at global address `addr` / at offset o of an LDS window, by two aligned 16-B
// loads (WEBSOCKET_BATCH_PAD and the windows' slack make the second one readable), and the
// header parsed from them.
__device__ __forceinline__ void ws_load16(uintptr_t addr, u64& h0, u64& h1) {
    const gu32x4* q = reinterpret_cast<const gu32x4*>(addr & ~(uintptr_t)15);
    ws_hdr_from32(q[0], q[1], (u32)(addr & 15), h0, h1);
}
__device__ __forceinline__ void ws_load16_win(const u32x4* win, u32 o, u64& h0, u64& h1) {
    ws_hdr_from32(win[o >> 4], win[(o >> 4) + 1], o & 15u, h0, h1);
}
__device__ __forceinline__ WsHdr ws_load_hdr(uintptr_t addr, u64 avail) {
    u64 h0, h1;
    ws_load16(addr, h0, h1);
    return ws_parse(h0, h1, avail);
}
__device__ __forceinline__ WsHdr ws_load_hdr_win(const u32x4* win, u32 o, u64 avail) {
    u64 h0, h1;
    ws_load16_win(win, o, h0, h1);
    return ws_parse(h0, h1, avail);
}

// Item of the unmask: w0 = P0 | rk[15:0] << 48, w1 = P1 | rk[31:16] << 48 — an origin-relative
// byte range [P0, P1) (< 2^48) and 32 bits riding on top (a frame's key, a segment's item count)
__device__ __forceinline__ u32x4 ws_item_pack(u64 p0, u64 p1, u32 rk) {
    const u64 w0 = p0 | ((u64)(rk & 0xFFFFu) << 48), w1 = p1 | ((u64)(rk >> 16) << 48);
    u32x4 q;
    q.x = (u32)w0; q.y = (u32)(w0 >> 32); q.z = (u32)w1; q.w = (u32)(w1 >> 32);
    return q;
}
__device__ __forceinline__ void ws_item_unpack(const u32x4 q, u64& p0, u64& p1, u32& rk) {
    const u64 w0 = (u64)q.x | ((u64)q.y << 32), w1 = (u64)q.z | ((u64)q.w << 32);
    p0 = w0 & 0xFFFFFFFFFFFFull;
    p1 = w1 & 0xFFFFFFFFFFFFull;
    rk = (u32)(w0 >> 48) | ((u32)(w1 >> 48) << 16);
}
// The frame h at origin-relative fo as the unmask sees it: its payload range (empty when it is
// not masked, so the items stay sorted) and its key rotated to the phase of 16-B-aligned chunks
__device__ __forceinline__ u32x4 ws_frame_item(const WsHdr& h, u64 fo) {
    const u64 p0 = fo + h.hdr;
    return ws_item_pack(p0, h.masked ? p0 + h.plen : p0, rotl32(h.key, 8u * (u32)(p0 & 3)));
}

// Pieces whose first byte is in [lo, hi) (origin-relative) point at `value` (segment << 32 | item;
// the raw stream is segment 0 of a table from piece 0, so its value is the item slot). Only
// pieces of the table [pbase, pend) exist. start, stride: lanes that write one range together,
// lane j the pieces j, j + stride, ...
__device__ __forceinline__ u64 ws_first_piece(u64 lo, u64 pbase) {
    const u64 p = (lo + (1ull << WS_PIECE_SHIFT) - 1) >> WS_PIECE_SHIFT;
    return p > pbase ? p : pbase;
}
__device__ __forceinline__ void ws_put_ptrs(u64* ptr, u64 pbase, u64 pend, u64 lo, u64 hi, u64 value, u64 start = 0,
                                            u64 stride = 1) {
    for (u64 p = ws_first_piece(lo, pbase) + start; (p << WS_PIECE_SHIFT) < hi && p < pend; p += stride)
        *gptr<u64>(ptr + (p - pbase)) = value;
}

// Descriptor as two 16-B stores (WebsocketFrameDesc_t layout).
__device__ __forceinline__ void ws_store_desc(WebsocketFrameDesc_t* d, u64 frame_off, const WsHdr& h) {
    const u64 dof = h.plen ? frame_off + h.hdr : WEBSOCKET_DATA_OFF_NULL;
    u32x4 q0, q1;
    q0.x = (u32)frame_off; q0.y = (u32)(frame_off >> 32); q0.z = (u32)dof; q0.w = (u32)(dof >> 32);
    q1.x = (u32)h.plen; q1.y = (u32)(h.plen >> 32); q1.z = (u32)h.ret;
    q1.w = (h.b0 >> 7) | ((h.b0 & 0x0Fu) << 8) | (h.masked << 16) | (h.hdr << 24);
    gu32x4* g = gptr<u32x4>(d);
    g[0] = q0;
    g[1] = q1;
}

// Everything the consumed frame h at `pos` of a raw stream (origin = pos + lead0) leaves behind
// as item `slot`: the item, the pointers of the pieces that start in it, and its descriptor (a
// ret == 0 frame has none). Returns the frame's end (origin-relative).
__device__ __forceinline__ u64 ws_emit_frame(const WsHdr& h, u64 pos, u64 lead0, u64 slot, WebsocketFrameDesc_t* desc,
                                             u32x4* items, u64* ptr, u64 pend) {
    const u64 fo = lead0 + pos, fe = fo + h.hdr + h.plen;
    *gptr<u32x4>(items + slot) = ws_frame_item(h, fo);
    ws_put_ptrs(ptr, 0, pend, fo, fe, slot);
    if (h.ret != 0) ws_store_desc(desc + slot, pos, h);
    return fe;
}
#endif  // __HIPCC__
