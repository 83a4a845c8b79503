// ws_handshake.h — the opening handshake's rule (websocketframe.c:16-108 over memfunc.c's strStr
// and strChr; include/wsframe_amd_handshake.h), defined once: the terminator, NUL and pattern
// tests on a window of bytes, the value skip and the value end, the SHA-1 block function, the
// message and padding layout of key || GUID, base64 of the digest and the response layout.
// Plain C++ — no HIP header, no AMDGPU builtin — so the kernels (ws_handshake.hip), the host entry
// point (websocketframeHandshakeHost) and a host driver (tests/c/handshake_host.cpp) build the
// same text and cannot drift apart.
//
// The reference's parse, restated as first positions. strStr(s, n, pat, m) returns the least i
// with i + m <= n, s[i, i + m) == pat and no NUL in s[0, i]; strChr(s, n, c) the least i < n with
// s[i] == c and no NUL in s[0, i). With
//   T  the least position of "\r\n\r\n" lying wholly inside the segment,
//   Z  the least position of a NUL byte,
//   K  the least position of "Sec-WebSocket-Key:" lying wholly inside the segment, P likewise
//      for "Sec-WebSocket-Protocol:",
// the request is incomplete (0) unless T exists and T < Z; then e = T, [0, e) holds no NUL, and
// the key header counts only if K + 18 <= e (a later match cannot count where the first does
// not), the protocol header only if P + 23 <= e. A value starts after the bytes that are <= 32 as
// a signed char and must start before e; it ends at the first '\r' in [start, e], which exists
// because e is one.
#pragma once
#include <stdint.h>

#include "../../include/wsframe_amd_handshake.h"

#ifdef __HIPCC__
#define WS_HS_FN __host__ __device__ inline __attribute__((always_inline))
#define WS_HS_UNROLL _Pragma("unroll")
#else
#define WS_HS_FN static inline
#define WS_HS_UNROLL
#endif

#define WS_HS_KEY_PAT_LEN 18u      // "Sec-WebSocket-Key:"
#define WS_HS_PROTO_PAT_LEN 23u    // "Sec-WebSocket-Protocol:"
#define WS_HS_GUID_LEN 36u
#define WS_HS_HEAD_LEN 97u         // the response up to and including "Sec-WebSocket-Accept: "
#define WS_HS_ACCEPT_LEN 28u
#define WS_HS_RESP_PLAIN 129u      // head + accept + "\r\n\r\n"
#define WS_HS_FIXED_PROTO 151u     // head + accept + "\r\nSec-WebSocket-Protocol: "; then the range and "\r\n\r\n"
#define WS_HS_FIXED_WORDS 38u      // dwords that cover the longer fixed part
#define WS_HS_MAX_SEG 0x80000000ull

// ------------------------------------------------------------------ the window tests

// bits [lo, hi) of a 16-bit chunk mask, for any signed lo, hi
WS_HS_FN uint32_t ws_hs_mask16(long long lo, long long hi) {
    const uint32_t l = lo < 0 ? 0u : (lo > 16 ? 16u : (uint32_t)lo), h = hi < 0 ? 0u : (hi > 16 ? 16u : (uint32_t)hi);
    return h > l ? ((1u << h) - 1u) & ~((1u << l) - 1u) : 0u;
}

// What the 16 positions of a chunk are, bit j for the position at chunk byte j: the start of
// "\r\n\r\n", a NUL byte, the start of "Sec-" (a candidate for either pattern). w0..w3 are the
// chunk's bytes and w4 the four after it (little-endian dwords). Positions [lo, hi_pat) may start
// a four-byte match (all four bytes inside the segment), positions [lo, hi_nul) are segment bytes.
struct WsHsChunk { uint32_t term, nul, sec; };
WS_HS_FN WsHsChunk ws_hs_chunk(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, long long lo,
                               long long hi_nul, long long hi_pat) {
    const uint32_t w[5] = {w0, w1, w2, w3, w4};
    WsHsChunk c = {0u, 0u, 0u};
    WS_HS_UNROLL
    for (int j = 0; j < 16; ++j) {
        const int q = j >> 2, r = 8 * (j & 3);
        const uint32_t win = r ? (w[q] >> r) | (w[q + 1] << (32 - r)) : w[q];
        c.term |= (uint32_t)(win == 0x0A0D0A0Du) << j;                 // "\r\n\r\n"
        c.sec |= (uint32_t)(win == 0x2D636553u) << j;                  // "Sec-"
        c.nul |= (uint32_t)((win & 0xFFu) == 0u) << j;
    }
    const uint32_t mp = ws_hs_mask16(lo, hi_pat);
    c.term &= mp;
    c.sec &= mp;
    c.nul &= ws_hs_mask16(lo, hi_nul);
    return c;
}

// The pattern that starts at p, of which `avail` bytes belong to the segment: 1 the key header's,
// 2 the protocol header's, 0 neither. Reads only bytes of the segment.
// Every byte is loaded before any is compared (no early exit), so on the device the loads are
// in flight together: one memory latency per candidate, not one per byte.
WS_HS_FN int ws_hs_pattern_at(const unsigned char* p, unsigned long long avail) {
    if (avail < WS_HS_KEY_PAT_LEN) return 0;
    const bool longer = avail >= WS_HS_PROTO_PAT_LEN;
    unsigned char b[WS_HS_PROTO_PAT_LEN];
    WS_HS_UNROLL
    for (int i = 0; i < (int)WS_HS_PROTO_PAT_LEN; ++i) b[i] = i < (int)WS_HS_KEY_PAT_LEN || longer ? p[i] : (unsigned char)0;
    const char* const key = "Sec-WebSocket-Key:";
    const char* const proto = "Sec-WebSocket-Protocol:";
    unsigned dk = 0, dp = 0;
    WS_HS_UNROLL
    for (int i = 0; i < (int)WS_HS_KEY_PAT_LEN; ++i) dk |= (unsigned)(b[i] ^ (unsigned char)key[i]);
    WS_HS_UNROLL
    for (int i = 0; i < (int)WS_HS_PROTO_PAT_LEN; ++i) dp |= (unsigned)(b[i] ^ (unsigned char)proto[i]);
    return dk == 0 ? 1 : (dp == 0 && longer ? 2 : 0);
}

// the value skip takes this byte (<= 32 as a signed char); the value ends at this byte
WS_HS_FN bool ws_hs_skips(unsigned char b) { return (signed char)b <= 32; }
WS_HS_FN bool ws_hs_ends(unsigned char b) { return b == '\r'; }

// 1 the request is complete with its terminator at T, 0 it is not (no terminator, or a NUL first)
WS_HS_FN int ws_hs_complete(uint32_t T, uint32_t Z) { return T != WEBSOCKET_HS_NONE && T < Z; }
// the header whose pattern of m bytes first matches at k counts
WS_HS_FN bool ws_hs_header_counts(uint32_t k, uint32_t m, uint32_t e) { return k != WEBSOCKET_HS_NONE && k + m <= e; }

// the response's length for a complete request; proto_off NONE: no protocol was parsed
WS_HS_FN uint32_t ws_hs_resp_len(uint32_t flags, uint32_t proto_off, uint32_t proto_len) {
    return (flags & WEBSOCKET_HS_ECHO_PROTOCOL) && proto_off != WEBSOCKET_HS_NONE && proto_len
               ? WS_HS_FIXED_PROTO + proto_len + 4u : WS_HS_RESP_PLAIN;
}

// The descriptor from the parse: ret <= 0 leaves the offsets at their rest values; the response
// flags follow from the lengths alone (has_resp: a response buffer was given).
WS_HS_FN WebsocketHandshakeDesc_t ws_hs_desc(int ret, uint32_t key_off, uint32_t key_len, uint32_t proto_off,
                                             uint32_t proto_len, uint32_t flags, bool has_resp, uint32_t resp_cap) {
    WebsocketHandshakeDesc_t d;
    d.ret = ret;
    d.key_off = ret > 0 ? key_off : 0u;
    d.key_len = ret > 0 ? key_len : 0u;
    d.proto_off = ret > 0 ? proto_off : WEBSOCKET_HS_NONE;
    d.proto_len = ret > 0 && proto_off != WEBSOCKET_HS_NONE ? proto_len : 0u;
    d.resp_len = ret > 0 ? ws_hs_resp_len(flags, d.proto_off, d.proto_len) : 0u;
    d.flags = ret > 0 && has_resp ? (d.resp_len > resp_cap ? WEBSOCKET_HS_RESP_NO_SPACE : WEBSOCKET_HS_RESP_WRITTEN) : 0u;
    d.reserved = 0u;
    return d;
}
WS_HS_FN WebsocketHandshakeDesc_t ws_hs_desc_seg_len() {
    WebsocketHandshakeDesc_t d = ws_hs_desc(-1, 0u, 0u, WEBSOCKET_HS_NONE, 0u, 0u, false, 0u);
    d.flags = WEBSOCKET_HS_ERR_SEG_LEN;
    return d;
}

// ------------------------------------------------------------------ SHA-1 of key || GUID

WS_HS_FN uint32_t ws_hs_rol(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

WS_HS_FN void ws_hs_sha1_init(uint32_t h[5]) {
    h[0] = 0x67452301u; h[1] = 0xEFCDAB89u; h[2] = 0x98BADCFEu; h[3] = 0x10325476u; h[4] = 0xC3D2E1F0u;
}

// One block. Every index into w is a compile-time constant once the loops are unrolled, so the
// schedule stays in registers on the device.
WS_HS_FN void ws_hs_sha1_block(uint32_t h[5], uint32_t w[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
    WS_HS_UNROLL
    for (int r = 0; r < 80; ++r) {
        uint32_t wr;
        if (r < 16) {
            wr = w[r & 15];
        } else {
            wr = ws_hs_rol(w[(r + 13) & 15] ^ w[(r + 8) & 15] ^ w[(r + 2) & 15] ^ w[r & 15], 1);
            w[r & 15] = wr;
        }
        uint32_t f, k;
        if (r < 20) { f = d ^ (b & (c ^ d)); k = 0x5A827999u; }
        else if (r < 40) { f = b ^ c ^ d; k = 0x6ED9EBA1u; }
        else if (r < 60) { f = (b & c) | (d & (b | c)); k = 0x8F1BBCDCu; }
        else { f = b ^ c ^ d; k = 0xCA62C1D6u; }
        const uint32_t t = ws_hs_rol(a, 5) + f + e + k + wr;
        e = d; d = c; c = ws_hs_rol(b, 30); b = a; a = t;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
}

// blocks of the padded message key || GUID: 0x80, zeros and the 8-byte bit length follow its
// key_len + 36 bytes, so the padding takes a further block from (key_len + 36) % 64 >= 56
WS_HS_FN uint32_t ws_hs_sha1_blocks(uint32_t key_len) { return 1u + (uint32_t)(((unsigned long long)key_len + 44u) / 64u); }

// byte i of the padded message (i < 64 * nblocks)
WS_HS_FN uint32_t ws_hs_msg_byte(const unsigned char* key, uint32_t key_len, uint32_t nblocks, unsigned long long i) {
    const unsigned long long n = (unsigned long long)key_len + WS_HS_GUID_LEN, total = 64ull * nblocks;
    if (i < key_len) return key[i];
    if (i < n) return (unsigned char)"258EAFA5-E914-47DA-95CA-C5AB0DC85B11"[i - key_len];
    if (i == n) return 0x80u;
    if (i >= total - 8u) return (uint32_t)((n * 8u) >> (8u * (total - 1u - i))) & 0xFFu;
    return 0u;
}

// the schedule words of block `blk` (big-endian)
WS_HS_FN void ws_hs_msg_block(const unsigned char* key, uint32_t key_len, uint32_t nblocks, uint32_t blk, uint32_t w[16]) {
    const unsigned long long base = 64ull * blk;
    WS_HS_UNROLL
    for (int t = 0; t < 16; ++t) {
        const unsigned long long i = base + 4u * (unsigned)t;
        w[t] = ws_hs_msg_byte(key, key_len, nblocks, i) << 24 | ws_hs_msg_byte(key, key_len, nblocks, i + 1) << 16 |
               ws_hs_msg_byte(key, key_len, nblocks, i + 2) << 8 | ws_hs_msg_byte(key, key_len, nblocks, i + 3);
    }
}

// ------------------------------------------------------------------ base64 of the digest

WS_HS_FN uint32_t ws_hs_b64_char(uint32_t v) {
    return v < 26u ? 'A' + v : (v < 52u ? 'a' + (v - 26u) : (v < 62u ? '0' + (v - 52u) : (v == 62u ? '+' : '/')));
}

// the 28 accept characters of the digest h, as 7 little-endian dwords (character i in byte i & 3
// of acc[i >> 2])
WS_HS_FN void ws_hs_accept(const uint32_t h[5], uint32_t acc[7]) {
    WS_HS_UNROLL
    for (int g = 0; g < 7; ++g) {
        // digest bytes 3g, 3g + 1, 3g + 2 (the last group has two: its fourth character is '=')
        uint32_t v = 0;
        WS_HS_UNROLL
        for (int k = 0; k < 3; ++k) {
            const int i = 3 * g + k;
            v = v << 8 | (i < 20 ? (h[(i < 20 ? i : 0) >> 2] >> (24 - 8 * (i & 3))) & 0xFFu : 0u);
        }
        acc[g] = ws_hs_b64_char(v >> 18) | ws_hs_b64_char((v >> 12) & 63u) << 8 | ws_hs_b64_char((v >> 6) & 63u) << 16 |
                 (g < 6 ? ws_hs_b64_char(v & 63u) : (uint32_t)'=') << 24;
    }
}

// ------------------------------------------------------------------ the response

// Byte i (< 151) of the response's fixed part: the head, the accept characters, then
// "\r\nSec-WebSocket-Protocol: " when a protocol line follows, else "\r\n\r\n" (i < 129).
WS_HS_FN uint32_t ws_hs_fixed_byte(int i, const uint32_t acc[7], bool with_proto) {
    if (i < (int)WS_HS_HEAD_LEN)
        return (unsigned char)"HTTP/1.1 101 Switching Protocols\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
                              "Sec-WebSocket-Accept: "[i];
    if (i < (int)(WS_HS_HEAD_LEN + WS_HS_ACCEPT_LEN)) {
        const int a = i - (int)WS_HS_HEAD_LEN;
        return (acc[a >> 2] >> (8 * (a & 3))) & 0xFFu;
    }
    const int t = i - (int)(WS_HS_HEAD_LEN + WS_HS_ACCEPT_LEN);
    const uint32_t plain = t < 4 ? (unsigned char)"\r\n\r\n"[t] : 0u;
    const uint32_t proto = t < 26 ? (unsigned char)"\r\nSec-WebSocket-Protocol: "[t] : 0u;
    return with_proto ? proto : plain;
}

// dword i (< WS_HS_FIXED_WORDS) of the fixed part, little-endian
WS_HS_FN uint32_t ws_hs_fixed_word(int i, const uint32_t acc[7], bool with_proto) {
    return ws_hs_fixed_byte(4 * i, acc, with_proto) | ws_hs_fixed_byte(4 * i + 1, acc, with_proto) << 8 |
           ws_hs_fixed_byte(4 * i + 2, acc, with_proto) << 16 | ws_hs_fixed_byte(4 * i + 3, acc, with_proto) << 24;
}

// ------------------------------------------------------------------ one segment, in sequence

// the value after the pattern of m bytes at k: false when the skip reaches e
WS_HS_FN bool ws_hs_value_seq(const unsigned char* buf, uint32_t k, uint32_t m, uint32_t e, uint32_t* off, uint32_t* len) {
    uint32_t p = k + m;
    while (p < e && ws_hs_skips(buf[p])) ++p;
    if (p >= e) return false;
    uint32_t q = p;
    while (q < e && !ws_hs_ends(buf[q])) ++q;       // buf[e] is '\r'
    *off = p;
    *len = q - p;
    return true;
}

// accept (28 characters + 4 zero bytes, as 8 dwords) of the key
WS_HS_FN void ws_hs_accept_of(const unsigned char* key, uint32_t key_len, uint32_t acc[8]) {
    uint32_t h[5], w[16];
    ws_hs_sha1_init(h);
    const uint32_t nb = ws_hs_sha1_blocks(key_len);
    for (uint32_t b = 0; b < nb; ++b) {
        ws_hs_msg_block(key, key_len, nb, b, w);
        ws_hs_sha1_block(h, w);
    }
    ws_hs_accept(h, acc);
    acc[7] = 0u;
}

// The whole rule for one segment buf[0, len) (WEBSOCKET_BATCH_PAD readable bytes follow it), chunk by
// chunk as the parse kernel does it, then accept and response. accept: 32 bytes, optional; resp:
// optional.
WS_HS_FN void ws_hs_one(const unsigned char* buf, unsigned long long len, uint32_t flags, WebsocketHandshakeDesc_t* hs,
                        unsigned char* accept, unsigned char* resp, uint32_t resp_cap) {
    if (len >= WS_HS_MAX_SEG) { *hs = ws_hs_desc_seg_len(); return; }
    const uint32_t n = (uint32_t)len;
    uint32_t T = WEBSOCKET_HS_NONE, Z = WEBSOCKET_HS_NONE, K = WEBSOCKET_HS_NONE, P = WEBSOCKET_HS_NONE;
    for (uint32_t cb = 0; cb < n && T == WEBSOCKET_HS_NONE && Z == WEBSOCKET_HS_NONE; cb += 16) {
        uint32_t w[5];
        for (int t = 0; t < 5; ++t)
            w[t] = (uint32_t)buf[cb + 4 * t] | (uint32_t)buf[cb + 4 * t + 1] << 8 | (uint32_t)buf[cb + 4 * t + 2] << 16 |
                   (uint32_t)buf[cb + 4 * t + 3] << 24;
        const WsHsChunk c = ws_hs_chunk(w[0], w[1], w[2], w[3], w[4], 0, (long long)n - cb, (long long)n - 3 - cb);
        for (uint32_t m = c.sec; m; m &= m - 1) {
            const uint32_t p = cb + (uint32_t)__builtin_ctz(m);
            const int kind = ws_hs_pattern_at(buf + p, n - p);
            if (kind == 1 && K == WEBSOCKET_HS_NONE) K = p;
            if (kind == 2 && P == WEBSOCKET_HS_NONE) P = p;
        }
        if (c.term) T = cb + (uint32_t)__builtin_ctz(c.term);
        if (c.nul) Z = cb + (uint32_t)__builtin_ctz(c.nul);
    }
    int ret = 0;
    uint32_t ko = 0, kl = 0, po = WEBSOCKET_HS_NONE, pl = 0;
    if (ws_hs_complete(T, Z)) {
        const uint32_t e = T;
        ret = -1;
        if (ws_hs_header_counts(K, WS_HS_KEY_PAT_LEN, e) && ws_hs_value_seq(buf, K, WS_HS_KEY_PAT_LEN, e, &ko, &kl)) {
            ret = (int)(e + 4u);
            if (!ws_hs_header_counts(P, WS_HS_PROTO_PAT_LEN, e) || !ws_hs_value_seq(buf, P, WS_HS_PROTO_PAT_LEN, e, &po, &pl)) {
                po = WEBSOCKET_HS_NONE;
                pl = 0;
            }
        }
    }
    *hs = ws_hs_desc(ret, ko, kl, po, pl, flags, resp != 0, resp_cap);
    if (ret <= 0 || (!accept && !(hs->flags & WEBSOCKET_HS_RESP_WRITTEN))) return;
    uint32_t acc[8];
    ws_hs_accept_of(buf + ko, kl, acc);
    if (accept)
        for (int i = 0; i < 32; ++i) accept[i] = (unsigned char)(acc[i >> 2] >> (8 * (i & 3)));
    if (!(hs->flags & WEBSOCKET_HS_RESP_WRITTEN)) return;
    const bool wp = hs->resp_len != WS_HS_RESP_PLAIN;
    const uint32_t fixed = wp ? WS_HS_FIXED_PROTO : WS_HS_RESP_PLAIN;
    for (uint32_t i = 0; i < fixed; ++i) resp[i] = (unsigned char)ws_hs_fixed_byte((int)i, acc, wp);
    if (wp) {
        for (uint32_t i = 0; i < pl; ++i) resp[fixed + i] = buf[po + i];
        for (uint32_t i = 0; i < 4; ++i) resp[fixed + pl + i] = (unsigned char)"\r\n\r\n"[i];
    }
}
