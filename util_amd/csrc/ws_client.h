// ws_client.h — the client side of the opening handshake (include/wsframe_amd_client.h), its
// rule defined once: the request's text and length, the byte checks, the key characters of a
// nonce and the accept value they must be answered with; the response's window tests (terminator,
// line ends, header candidates), the header names, the status line, the order of the checks and
// the descriptor. Plain C++ — no HIP header, no AMDGPU builtin — so the kernels (ws_client.hip),
// the host entry points and a host driver (tests/c/client_host.cpp) build the same text and
// cannot drift apart. SHA-1, base64 and the 16-bit chunk mask are ws_handshake.h's.
//
// The response's parse as positions. With n = min(seg_len, max_head or seg_len) and T the least
// position of "\r\n\r\n" lying wholly inside [0, n), the response is complete iff T exists; e = T.
// Every "\r\n" at j < e ends a line and starts the next at j + 2; a line that starts at p is the
// header `name` iff [p, p + len(name) + 1) folds to name ':' and p + len(name) + 1 <= e: the five
// names hold no ':', CR, SP or HT, so that colon is the line's first, the name is everything before
// it and no line end lies inside. Its value runs from there to the next "\r\n", which exists at or
// before e because e is one.
#pragma once
#include <stdint.h>

#include "../../include/wsframe_amd_client.h"
#include "ws_handshake.h"

#define WS_CL_MAX_SEG 0x80000000ull
#define WS_CL_KEY_LEN 24u
#define WS_CL_NAME_MAX 25u          // "sec-websocket-extensions:"

enum { WS_CL_H_NONE = 0, WS_CL_H_UPGRADE, WS_CL_H_CONNECTION, WS_CL_H_ACCEPT, WS_CL_H_EXTENSIONS, WS_CL_H_PROTOCOL };

// ------------------------------------------------------------------ bytes

WS_HS_FN uint32_t ws_cl_fold(uint32_t b) { return b - 'A' < 26u ? b | 0x20u : b; }      // A-Z only
WS_HS_FN bool ws_cl_ws(uint32_t b) { return b == ' ' || b == '\t'; }
WS_HS_FN bool ws_cl_digit(uint32_t b) { return b - '0' < 10u; }
// what the request may not carry: the path ends at the first space of the request line, and no
// field may bring a control byte (CR and LF among them) into the request
WS_HS_FN bool ws_cl_bad_path_byte(uint32_t b) { return b <= 0x20u || b == 0x7Fu; }
WS_HS_FN bool ws_cl_bad_field_byte(uint32_t b) { return b < 0x20u || b == 0x7Fu; }

// byte i of "websocket" (i < 9) and of "upgrade" (i < 7), for a lane that compares its own byte
WS_HS_FN uint32_t ws_cl_websocket_byte(uint32_t i) {
    return i < 8u ? (uint32_t)(0x656B636F73626577ull >> (8u * i)) & 0xFFu : (uint32_t)'t';
}
WS_HS_FN uint32_t ws_cl_upgrade_byte(uint32_t i) { return (uint32_t)(0x0065646172677075ull >> (8u * (i & 7u))) & 0xFFu; }

// ------------------------------------------------------------------ the request

#define WS_CL_R_GET "GET "
#define WS_CL_R_HTTP " HTTP/1.1\r\n"
#define WS_CL_R_HOST "Host: "
#define WS_CL_R_FIXED "Upgrade: websocket\r\nConnection: Upgrade\r\nSec-WebSocket-Version: 13\r\nSec-WebSocket-Key: "
#define WS_CL_R_PROTO "Sec-WebSocket-Protocol: "
#define WS_CL_R_EOL "\r\n"
#define WS_CL_LEN(s) ((uint32_t)sizeof(s) - 1u)
#define WS_CL_LIT(o, s)                                                                        \
    do {                                                                                       \
        WS_HS_UNROLL                                                                           \
        for (int i_ = 0; i_ < (int)WS_CL_LEN(s); ++i_) (o).put((uint32_t)(unsigned char)(s)[i_]); \
    } while (0)

// the key characters' offset in the request and the request's length (64-bit: three lengths of
// up to 2^32 - 1 each)
WS_HS_FN unsigned long long ws_cl_key_off(uint32_t path_len, uint32_t host_len) {
    return (unsigned long long)WS_CL_LEN(WS_CL_R_GET) + path_len + WS_CL_LEN(WS_CL_R_HTTP) +
           (host_len ? (unsigned long long)WS_CL_LEN(WS_CL_R_HOST) + host_len + WS_CL_LEN(WS_CL_R_EOL) : 0ull) +
           WS_CL_LEN(WS_CL_R_FIXED);
}
WS_HS_FN unsigned long long ws_cl_req_len(uint32_t path_len, uint32_t proto_len, uint32_t host_len) {
    return ws_cl_key_off(path_len, host_len) + WS_CL_KEY_LEN + WS_CL_LEN(WS_CL_R_EOL) +
           (proto_len ? (unsigned long long)WS_CL_LEN(WS_CL_R_PROTO) + proto_len + WS_CL_LEN(WS_CL_R_EOL) : 0ull) +
           WS_CL_LEN(WS_CL_R_EOL);
}

// ERR_BYTES or 0 for the three fields (absent ones have length 0)
WS_HS_FN uint32_t ws_cl_check_bytes(const unsigned char* path, uint32_t path_len, const unsigned char* proto,
                                    uint32_t proto_len, const unsigned char* host, uint32_t host_len) {
    uint32_t bad = 0;
    for (uint32_t i = 0; i < path_len; ++i) bad |= (uint32_t)ws_cl_bad_path_byte(path[i]);
    for (uint32_t i = 0; i < proto_len; ++i) bad |= (uint32_t)ws_cl_bad_field_byte(proto[i]);
    for (uint32_t i = 0; i < host_len; ++i) bad |= (uint32_t)ws_cl_bad_field_byte(host[i]);
    return bad ? WEBSOCKET_CLI_ERR_BYTES : 0u;
}

// the 24 key characters of the 16 nonce bytes (little-endian dwords, byte i in nonce[i >> 2]), as
// 6 little-endian dwords: one per base64 group, the last group "xx=="
WS_HS_FN void ws_cl_key(const uint32_t nonce[4], uint32_t key[6]) {
    WS_HS_UNROLL
    for (int g = 0; g < 6; ++g) {
        uint32_t v = 0;
        WS_HS_UNROLL
        for (int k = 0; k < 3; ++k) {
            const int i = 3 * g + k;
            v = v << 8 | (i < 16 ? (nonce[(i < 16 ? i : 0) >> 2] >> (8 * (i & 3))) & 0xFFu : 0u);
        }
        key[g] = ws_hs_b64_char(v >> 18) | ws_hs_b64_char((v >> 12) & 63u) << 8 |
                 (g < 5 ? ws_hs_b64_char((v >> 6) & 63u) : (uint32_t)'=') << 16 |
                 (g < 5 ? ws_hs_b64_char(v & 63u) : (uint32_t)'=') << 24;
    }
}

WS_HS_FN uint32_t ws_cl_bswap(uint32_t x) { return x << 24 | (x & 0xFF00u) << 8 | (x >> 8 & 0xFF00u) | x >> 24; }

// base64(SHA-1(key || GUID)) for a key of 24 characters, as 28 characters + 4 zero bytes in 8
// dwords: the message's 60 bytes and its 0x80 fill the first block, the bit length (480) ends the
// second, so every schedule word is a register or a constant
WS_HS_FN void ws_cl_expect(const uint32_t key[6], uint32_t acc[8]) {
    uint32_t h[5], w[16];
    ws_hs_sha1_init(h);
    WS_HS_UNROLL
    for (int t = 0; t < 16; ++t) {
        if (t < 6) {
            w[t] = ws_cl_bswap(key[t]);
        } else {
            const unsigned long long i = 4ull * (unsigned)t;          // (key bytes are never asked for: i >= 24)
            w[t] = ws_hs_msg_byte((const unsigned char*)0, WS_CL_KEY_LEN, 2u, i) << 24 |
                   ws_hs_msg_byte((const unsigned char*)0, WS_CL_KEY_LEN, 2u, i + 1) << 16 |
                   ws_hs_msg_byte((const unsigned char*)0, WS_CL_KEY_LEN, 2u, i + 2) << 8 |
                   ws_hs_msg_byte((const unsigned char*)0, WS_CL_KEY_LEN, 2u, i + 3);
        }
    }
    ws_hs_sha1_block(h, w);
    WS_HS_UNROLL
    for (int t = 0; t < 16; ++t) w[t] = t == 15 ? 8u * (WS_CL_KEY_LEN + WS_HS_GUID_LEN) : 0u;
    ws_hs_sha1_block(h, w);
    ws_hs_accept(h, acc);
    acc[7] = 0u;
}

// The request's bytes, in order, into a sink with put(byte): the two templates' text (and the
// Host line after the request line where a host is given). One definition for the host's byte
// writer and the kernel's 16-B funnel.
template <class Sink>
WS_HS_FN void ws_cl_emit_request(Sink& o, const unsigned char* path, uint32_t path_len, const unsigned char* proto,
                                 uint32_t proto_len, const unsigned char* host, uint32_t host_len, const uint32_t key[6]) {
    WS_CL_LIT(o, WS_CL_R_GET);
    for (uint32_t i = 0; i < path_len; ++i) o.put(path[i]);
    WS_CL_LIT(o, WS_CL_R_HTTP);
    if (host_len) {
        WS_CL_LIT(o, WS_CL_R_HOST);
        for (uint32_t i = 0; i < host_len; ++i) o.put(host[i]);
        WS_CL_LIT(o, WS_CL_R_EOL);
    }
    WS_CL_LIT(o, WS_CL_R_FIXED);
    WS_HS_UNROLL
    for (int i = 0; i < (int)WS_CL_KEY_LEN; ++i) o.put((key[i >> 2] >> (8 * (i & 3))) & 0xFFu);
    WS_CL_LIT(o, WS_CL_R_EOL);
    if (proto_len) {
        WS_CL_LIT(o, WS_CL_R_PROTO);
        for (uint32_t i = 0; i < proto_len; ++i) o.put(proto[i]);
        WS_CL_LIT(o, WS_CL_R_EOL);
    }
    WS_CL_LIT(o, WS_CL_R_EOL);
}

// The request descriptor from the lengths alone. err: ERR_RANGE / ERR_BYTES bits (then nothing
// is written); has_req: a request buffer was given.
WS_HS_FN WebsocketClientReqDesc_t ws_cl_req_desc(uint32_t err, uint32_t path_len, uint32_t proto_len, uint32_t host_len,
                                                 bool has_req, uint32_t req_cap) {
    WebsocketClientReqDesc_t d;
    const unsigned long long n = ws_cl_req_len(path_len, proto_len, host_len);
    if (path_len == 0u || n > 0xFFFFFFFFull) err |= WEBSOCKET_CLI_ERR_RANGE;
    d.req_len = err ? 0u : (uint32_t)n;
    d.key_off = err ? 0u : (uint32_t)ws_cl_key_off(path_len, host_len);
    d.flags = err ? err : (has_req ? (n > req_cap ? WEBSOCKET_CLI_REQ_NO_SPACE : WEBSOCKET_CLI_REQ_WRITTEN) : 0u);
    d.reserved = 0u;
    return d;
}

#ifdef __HIPCC__
#define WS_CL_MEMBER __host__ __device__ inline __attribute__((always_inline))
#else
#define WS_CL_MEMBER inline
#endif
struct WsClByteSink {
    unsigned char* p;
    WS_CL_MEMBER void put(uint32_t b) { *p++ = (unsigned char)b; }
};

// The whole request rule for one connection, byte by byte. req: optional.
WS_HS_FN void ws_cl_request_one(const unsigned char* path, uint32_t path_len, const unsigned char* proto,
                                uint32_t proto_len, const unsigned char* host, uint32_t host_len,
                                const unsigned char nonce[16], unsigned char* req, uint32_t req_cap,
                                unsigned char expect[32], WebsocketClientReqDesc_t* rd) {
    const uint32_t err = ws_cl_check_bytes(path, path_len, proto, proto_len, host, host_len);
    *rd = ws_cl_req_desc(err, path_len, proto_len, host_len, req != 0, req_cap);
    if (rd->flags & (WEBSOCKET_CLI_ERR_RANGE | WEBSOCKET_CLI_ERR_BYTES)) return;
    uint32_t nw[4], key[6], acc[8];
    for (int i = 0; i < 4; ++i)
        nw[i] = (uint32_t)nonce[4 * i] | (uint32_t)nonce[4 * i + 1] << 8 | (uint32_t)nonce[4 * i + 2] << 16 |
                (uint32_t)nonce[4 * i + 3] << 24;
    ws_cl_key(nw, key);
    ws_cl_expect(key, acc);
    for (int i = 0; i < 32; ++i) expect[i] = (unsigned char)(acc[i >> 2] >> (8 * (i & 3)));
    if (!(rd->flags & WEBSOCKET_CLI_REQ_WRITTEN)) return;
    WsClByteSink o = {req};
    ws_cl_emit_request(o, path, path_len, proto, proto_len, host, host_len, key);
}

// ------------------------------------------------------------------ the response: window tests

// What the 16 positions of a chunk are, bit j for the position at chunk byte j: the start of
// "\r\n\r\n", the start of a "\r\n", and a "\r\n" after which a line begins whose first byte folds
// to 'u', 'c' or 's' (a candidate for the five header names; that byte is looked at, not trusted:
// the name test reads only bytes of the response). w0..w3 are the chunk's bytes and w4 the four
// after it. Positions [lo, hi) are the response's bytes: a pattern counts only wholly inside.
struct WsClChunk { uint32_t term, crlf, cand; };
WS_HS_FN WsClChunk ws_cl_chunk(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, long long lo, long long hi) {
    const uint32_t w[5] = {w0, w1, w2, w3, w4};
    WsClChunk c = {0u, 0u, 0u};
    WS_HS_UNROLL
    for (int j = 0; j < 16; ++j) {
        const int q = j >> 2, r = 8 * (j & 3);
        const uint32_t win = r ? (w[q] >> r) | (w[q + 1] << (32 - r)) : w[q];
        const uint32_t f = ws_cl_fold((win >> 16) & 0xFFu);
        const bool eol = (win & 0xFFFFu) == 0x0A0Du;
        c.term |= (uint32_t)(win == 0x0A0D0A0Du) << j;
        c.crlf |= (uint32_t)eol << j;
        c.cand |= (uint32_t)(eol && (f == 'u' || f == 'c' || f == 's')) << j;
    }
    c.term &= ws_hs_mask16(lo, hi - 3);
    c.crlf &= ws_hs_mask16(lo, hi - 1);
    c.cand &= ws_hs_mask16(lo, hi - 1);
    return c;
}

WS_HS_FN uint32_t ws_cl_name_len(int kind) {     // with its ':'
    return kind == WS_CL_H_UPGRADE ? 8u : (kind == WS_CL_H_CONNECTION ? 11u : (kind == WS_CL_H_ACCEPT ? 21u :
           (kind == WS_CL_H_EXTENSIONS ? 25u : 23u)));
}

// The header whose name and ':' start at p, of which `avail` bytes belong to [0, e): WS_CL_H_*.
// Reads only those bytes. Every byte is loaded before any is compared, so on the device the
// loads are in flight together: one memory latency per candidate.
WS_HS_FN int ws_cl_name_at(const unsigned char* p, unsigned long long avail) {
    uint32_t b[WS_CL_NAME_MAX];
    WS_HS_UNROLL
    for (int i = 0; i < (int)WS_CL_NAME_MAX; ++i) b[i] = (unsigned)i < avail ? (uint32_t)p[i] : 0u;
    const char* const nu = "upgrade:";
    const char* const nc = "connection:";
    const char* const na = "sec-websocket-accept:";
    const char* const ne = "sec-websocket-extensions:";
    const char* const np = "sec-websocket-protocol:";
    uint32_t du = 0, dc = 0, da = 0, de = 0, dp = 0;
    WS_HS_UNROLL
    for (int i = 0; i < (int)WS_CL_NAME_MAX; ++i) {
        const uint32_t f = ws_cl_fold(b[i]);
        if (i < 8) du |= f ^ (unsigned char)nu[i];
        if (i < 11) dc |= f ^ (unsigned char)nc[i];
        if (i < 21) da |= f ^ (unsigned char)na[i];
        if (i < 25) de |= f ^ (unsigned char)ne[i];
        if (i < 23) dp |= f ^ (unsigned char)np[i];
    }
    // (a byte past `avail` reads as 0 and matches no name byte, so a short line matches nothing)
    return du == 0 ? WS_CL_H_UPGRADE : (dc == 0 ? WS_CL_H_CONNECTION : (da == 0 ? WS_CL_H_ACCEPT :
           (de == 0 ? WS_CL_H_EXTENSIONS : (dp == 0 ? WS_CL_H_PROTOCOL : WS_CL_H_NONE))));
}

// The status line from its first 13 bytes (f[i] = 0 for i >= l0, its length): true iff it starts
// "HTTP/1.1 101" with its end or a space after it; *status the three digits of an "HTTP/1.d ddd" line.
WS_HS_FN bool ws_cl_status_line(const uint32_t f[13], uint32_t l0, uint32_t* status) {
    const char* const lit = "HTTP/1.1 101";
    uint32_t d7 = 0, d12 = 0;
    WS_HS_UNROLL
    for (int i = 0; i < 12; ++i) {
        if (i < 7) d7 |= f[i] ^ (unsigned char)lit[i];
        d12 |= f[i] ^ (unsigned char)lit[i];
    }
    const bool line = l0 >= 12u && d7 == 0 && ws_cl_digit(f[7]) && f[8] == ' ' && ws_cl_digit(f[9]) && ws_cl_digit(f[10]) &&
                      ws_cl_digit(f[11]);
    *status = line ? (f[9] - '0') * 100u + (f[10] - '0') * 10u + (f[11] - '0') : 0u;
    return l0 >= 12u && d12 == 0 && (l0 == 12u || f[12] == ' ');
}

// what the sweep over the headers leaves: which checks passed, and the two reported ranges
struct WsClHeaders {
    bool have_up, up_ok, conn_ok, have_acc, acc_ok, ext_bad;
    uint32_t acc_off, nproto, proto_off, proto_len;
};
WS_HS_FN WsClHeaders ws_cl_headers_init() {
    WsClHeaders h = {false, false, false, false, false, false, WEBSOCKET_CLI_NONE, 0u, WEBSOCKET_CLI_NONE, 0u};
    return h;
}

// the one protocol header that may be judged against the offered list
WS_HS_FN bool ws_cl_proto_judged(const WsClHeaders& h) { return h.nproto == 1u && h.proto_len != 0u; }

// The descriptor of a complete response (terminator at e): the checks in the RFC's order.
// proto_ok: the judged protocol value is an offered element.
WS_HS_FN WebsocketClientVerifyDesc_t ws_cl_vdesc(uint32_t e, bool status_ok, uint32_t status, const WsClHeaders& h,
                                                 bool proto_ok) {
    WebsocketClientVerifyDesc_t d;
    d.reason = !status_ok ? WEBSOCKET_CLI_REASON_STATUS
             : !(h.have_up && h.up_ok) ? WEBSOCKET_CLI_REASON_UPGRADE
             : !h.conn_ok ? WEBSOCKET_CLI_REASON_CONNECTION
             : !(h.have_acc && h.acc_ok) ? WEBSOCKET_CLI_REASON_ACCEPT
             : h.ext_bad ? WEBSOCKET_CLI_REASON_EXTENSION
             : (h.nproto && !(ws_cl_proto_judged(h) && proto_ok)) ? WEBSOCKET_CLI_REASON_PROTOCOL : WEBSOCKET_CLI_OK;
    d.ret = d.reason ? -1 : (int)(e + 4u);
    d.status = status;
    d.proto_off = d.ret > 0 && h.nproto ? h.proto_off : WEBSOCKET_CLI_NONE;
    d.proto_len = d.ret > 0 && h.nproto ? h.proto_len : 0u;
    d.accept_off = h.have_acc ? h.acc_off : WEBSOCKET_CLI_NONE;
    d.flags = 0u;
    d.reserved = 0u;
    return d;
}
// of a response that is not complete: ret 0, or -1 with TOO_LONG / the ERR_SEG_LEN flag
WS_HS_FN WebsocketClientVerifyDesc_t ws_cl_vdesc_rest(int ret, uint32_t reason, uint32_t flags) {
    WebsocketClientVerifyDesc_t d;
    d.ret = ret; d.reason = reason; d.status = 0u;
    d.proto_off = WEBSOCKET_CLI_NONE; d.proto_len = 0u; d.accept_off = WEBSOCKET_CLI_NONE;
    d.flags = flags; d.reserved = 0u;
    return d;
}
WS_HS_FN WebsocketClientVerifyDesc_t ws_cl_vdesc_incomplete(unsigned long long seg_len, uint32_t max_head) {
    return max_head && seg_len >= max_head ? ws_cl_vdesc_rest(-1, WEBSOCKET_CLI_REASON_TOO_LONG, 0u)
                                           : ws_cl_vdesc_rest(0, WEBSOCKET_CLI_OK, 0u);
}
// the bytes of the segment that may be looked at
WS_HS_FN uint32_t ws_cl_head_len(uint32_t seg_len, uint32_t max_head) { return max_head && max_head < seg_len ? max_head : seg_len; }

// ------------------------------------------------------------------ one response, in sequence

// The field that starts at st: its delimiter (the first "\r\n" wholly inside [st, n) when crlf,
// else the first ',' in [st, n); none: n) and its bytes trimmed of SP and HT, [*a, *b) (an empty
// field: both at the delimiter).
WS_HS_FN uint32_t ws_cl_field_seq(const unsigned char* s, uint32_t st, uint32_t n, bool crlf, uint32_t* a, uint32_t* b) {
    uint32_t d = st;
    while (d < n && !(crlf ? (d + 1u < n && s[d] == '\r' && s[d + 1u] == '\n') : s[d] == ',')) ++d;
    uint32_t x = st, y = d;
    while (x < y && ws_cl_ws(s[x])) ++x;
    while (y > x && ws_cl_ws(s[y - 1u])) --y;
    *a = x < y ? x : d;
    *b = x < y ? y : d;
    return d;
}

// some comma-separated element of list[a, b), trimmed, equals t[0, tlen) (fold: after folding the
// element's bytes; t is lower case then)
WS_HS_FN bool ws_cl_list_has_seq(const unsigned char* list, uint32_t a, uint32_t b, const unsigned char* t, uint32_t tlen,
                                 bool fold) {
    for (uint32_t cur = a;;) {
        uint32_t x, y;
        const uint32_t d = ws_cl_field_seq(list, cur, b, false, &x, &y);
        if (y - x == tlen) {
            uint32_t diff = 0;
            for (uint32_t i = 0; i < tlen; ++i) diff |= (fold ? ws_cl_fold(list[x + i]) : (uint32_t)list[x + i]) ^ t[i];
            if (!diff) return true;
        }
        if (d >= b) return false;
        cur = d + 1u;
    }
}

// The whole verify rule for one segment buf[0, len) (WEBSOCKET_BATCH_PAD readable bytes follow it).
// offered: the offered list or NULL.
WS_HS_FN void ws_cl_verify_one(const unsigned char* buf, unsigned long long len, const unsigned char* expect,
                               const unsigned char* offered, uint32_t offered_len, uint32_t max_head,
                               WebsocketClientVerifyDesc_t* cv) {
    if (len >= WS_CL_MAX_SEG) { *cv = ws_cl_vdesc_rest(-1, WEBSOCKET_CLI_OK, WEBSOCKET_CLI_ERR_SEG_LEN); return; }
    const uint32_t n = ws_cl_head_len((uint32_t)len, max_head);
    uint32_t T = WEBSOCKET_CLI_NONE, L0 = WEBSOCKET_CLI_NONE;
    WsClHeaders h = ws_cl_headers_init();
    // chunk by chunk, as the kernel's lanes see the bytes: a terminator ends the sweep, and the
    // chunk's candidates count up to it
    for (uint32_t cb = 0; cb < n && T == WEBSOCKET_CLI_NONE; cb += 16) {
        uint32_t w[5];
        for (int t = 0; t < 5; ++t)
            w[t] = (uint32_t)buf[cb + 4 * t] | (uint32_t)buf[cb + 4 * t + 1] << 8 | (uint32_t)buf[cb + 4 * t + 2] << 16 |
                   (uint32_t)buf[cb + 4 * t + 3] << 24;
        const WsClChunk c = ws_cl_chunk(w[0], w[1], w[2], w[3], w[4], 0, (long long)n - cb);
        if (c.term) T = cb + (uint32_t)__builtin_ctz(c.term);
        if (c.crlf && L0 == WEBSOCKET_CLI_NONE) L0 = cb + (uint32_t)__builtin_ctz(c.crlf);
        const uint32_t lim = T != WEBSOCKET_CLI_NONE ? T : n;
        for (uint32_t m = c.cand; m; m &= m - 1) {
            const uint32_t p = cb + (uint32_t)__builtin_ctz(m) + 2u;
            if (p + 8u > lim) continue;
            const int kind = ws_cl_name_at(buf + p, lim - p);
            if (!kind) continue;
            uint32_t a, b;
            ws_cl_field_seq(buf, p + ws_cl_name_len(kind), n, true, &a, &b);
            if (kind == WS_CL_H_UPGRADE && !h.have_up) {
                h.have_up = true;
                h.up_ok = b - a == 9u;
                for (uint32_t i = 0; i < 9u && h.up_ok; ++i) h.up_ok = ws_cl_fold(buf[a + i]) == ws_cl_websocket_byte(i);
            } else if (kind == WS_CL_H_CONNECTION && !h.conn_ok) {
                unsigned char up[7];
                for (uint32_t i = 0; i < 7u; ++i) up[i] = (unsigned char)ws_cl_upgrade_byte(i);
                h.conn_ok = ws_cl_list_has_seq(buf, a, b, up, 7u, true);
            } else if (kind == WS_CL_H_ACCEPT && !h.have_acc) {
                h.have_acc = true;
                h.acc_off = a;
                h.acc_ok = b - a == WS_HS_ACCEPT_LEN;
                for (uint32_t i = 0; i < WS_HS_ACCEPT_LEN && h.acc_ok; ++i) h.acc_ok = buf[a + i] == expect[i];
            } else if (kind == WS_CL_H_EXTENSIONS) {
                h.ext_bad = h.ext_bad || b > a;
            } else if (kind == WS_CL_H_PROTOCOL) {
                if (h.nproto++ == 0u) { h.proto_off = a; h.proto_len = b - a; }
            }
        }
    }
    if (T == WEBSOCKET_CLI_NONE) { *cv = ws_cl_vdesc_incomplete(len, max_head); return; }
    uint32_t f[13], status;
    for (uint32_t i = 0; i < 13u; ++i) f[i] = i < L0 ? (uint32_t)buf[i] : 0u;
    const bool status_ok = ws_cl_status_line(f, L0, &status);
    const bool proto_ok = ws_cl_proto_judged(h) && offered && offered_len &&
                          ws_cl_list_has_seq(offered, 0u, offered_len, buf + h.proto_off, h.proto_len, false);
    *cv = ws_cl_vdesc(T, status_ok, status, h, proto_ok);
}
