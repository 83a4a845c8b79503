// ws_deflate.h — the rule of websocketframeBatchDeflateDevice and websocketframeDeflateHost
// (include/wsframe_amd_compress.h), defined once: how a message body becomes a permessage-deflate
// body (one fixed-Huffman block of LZ77 tokens, closed by an empty stored block's header bits), the
// verdict (DEFLATED, PLAIN, ERR_OUT_SPACE) and what is written to the room. Plain C++ — no HIP
// header, no AMDGPU builtin — so the kernel (ws_deflate.hip), the host entry point and a CPU test
// (tests/test_deflate_host.py) compile the same text.
//
// The rule is positional: nothing in it depends on the order in which the 64 positions of a group
// are worked on, so one wavefront (a position per lane) and the host (a loop over the positions)
// write the same bytes. A message is taken in groups of WS_DEF_GROUP = 64 consecutive positions:
//   lookup   position p with 4 bytes left hashes them (ws_def_hash, hbits from the message's
//            length: 8 to 11 bits, the smallest table that has a slot per byte) and reads the
//            table as it stood before the group: the candidate is the last position inserted at
//            that slot, at distance d = p - candidate. 1 <= d <= 32,768 and d <= p (never before
//            the message's first byte), else there is none. The match length is the count of equal
//            bytes from p and p - d on, at most min(258, len - p); below WS_DEF_MINMATCH = 4 it is
//            no match. Positions that the previous group's last match covers look nothing up.
//   insert   then every position of the group with 4 bytes left is inserted, and the highest
//            position wins a slot (covered positions included: the table stays fresh in a run);
//   choose   greedy, first position first: from the first uncovered position on, a position with
//            a match emits it and covers its length, any other emits its byte as a literal;
//   pack     tokens in position order, fixed Huffman codes (RFC 1951 section 3.2.6): a token's bits
//            (at most 31) land at the exclusive prefix sum of the token lengths before it.
// The stream is: the block header (BFINAL 0, BTYPE 01), the tokens, the end-of-block code, 000 (an
// empty stored block's header), zero padding to the byte. enc_len is its length in bytes.
//
// Written against an Io: NL, l0() and l1() the positions of a group this caller holds (the host all
// 64, a lane its own), lane() and lanes() its share of a cooperative loop, uni() a value every
// caller holds alike, sync() between a store and another caller's load, ld8/ld32 body bytes,
// put32/max32/or32 table and staging words, ballot/bcast/scan across the group's positions,
// out_word/out_byte the room, phase() the room's address modulo 4 and copy() the PLAIN fallback.
// The staging buffer holds the stream from a 4-byte boundary of the room's address on (phase()), so
// whole words leave as aligned stores and only the room's ends are written byte by byte; which
// bytes are written does not depend on the phase.
#pragma once
#include <stdint.h>

#include "../../include/wsframe_amd_compress.h"

#ifdef __HIPCC__
#define WS_DEF_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define WS_DEF_FN static inline
#endif

typedef unsigned long long wsdef_u64;
typedef unsigned int wsdef_u32;

#define WS_DEF_GROUP 64u
#define WS_DEF_MINMATCH 4u
#define WS_DEF_MAXMATCH 258u
#define WS_DEF_MAXDIST 32768u
#define WS_DEF_HBITS_MIN 8u
#define WS_DEF_HBITS_MAX 11u
#define WS_DEF_EMPTY 0xFFFFFFFFu         // a table slot before its first insert (distance p + 1: never a candidate)
#define WS_DEF_STAGE 66u                 // staging words: 31 carried bits + 64 tokens of at most 31 bits, and a spill word

struct WsDefWork {                       // one caller group's scratch: 8,456 bytes
    wsdef_u32 tab[1u << WS_DEF_HBITS_MAX];
    wsdef_u32 stg[WS_DEF_STAGE];
};

WS_DEF_FN wsdef_u32 ws_def_hbits(wsdef_u64 len) {
    wsdef_u32 b = WS_DEF_HBITS_MIN;
    while (b < WS_DEF_HBITS_MAX && (1ull << b) < len) ++b;
    return b;
}
WS_DEF_FN wsdef_u32 ws_def_hash(wsdef_u32 four, wsdef_u32 hbits) { return (four * 0x9E3779B1u) >> (32u - hbits); }

// the low n bits of v, reversed (Huffman codes go out most significant bit first)
WS_DEF_FN wsdef_u32 ws_def_rev(wsdef_u32 v, wsdef_u32 n) {
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32u - n);
}
WS_DEF_FN wsdef_u32 ws_def_log2(wsdef_u32 v) { return 31u - (wsdef_u32)__builtin_clz(v); }   // v > 0

// a literal's bits in stream order; returns their count (8 or 9)
WS_DEF_FN wsdef_u32 ws_def_literal(wsdef_u32 b, wsdef_u32* bits) {
    if (b < 144u) {
        *bits = ws_def_rev(0x30u + b, 8);
        return 8;
    }
    *bits = ws_def_rev(0x190u + (b - 144u), 9);
    return 9;
}
// a match's bits in stream order: length code, its extra bits, distance code, its extra bits; at most 31
WS_DEF_FN wsdef_u32 ws_def_match(wsdef_u32 mlen, wsdef_u32 dist, wsdef_u32* bits) {
    const wsdef_u32 l = mlen - 3u;
    wsdef_u32 sym, le = 0, lx = 0;
    if (mlen == WS_DEF_MAXMATCH) {
        sym = 285;
    } else if (l < 8u) {
        sym = 257u + l;
    } else {
        le = ws_def_log2(l) - 2u;
        sym = 261u + 4u * le + ((l >> le) & 3u);
        lx = l & ((1u << le) - 1u);
    }
    wsdef_u32 n = sym < 280u ? 7u : 8u;
    wsdef_u32 v = sym < 280u ? ws_def_rev(sym - 256u, 7) : ws_def_rev(0xC0u + (sym - 280u), 8);
    v |= lx << n;
    n += le;
    const wsdef_u32 d = dist - 1u;
    wsdef_u32 dsym = d, de = 0, dx = 0;
    if (d >= 4u) {
        de = ws_def_log2(d) - 1u;
        dsym = 2u * de + 2u + ((d >> de) & 1u);
        dx = d & ((1u << de) - 1u);
    }
    v |= ws_def_rev(dsym, 5) << n;
    n += 5u;
    v |= dx << n;
    n += de;
    *bits = v;
    return n;
}

WS_DEF_FN wsdef_u64 ws_def_range(wsdef_u32 a, wsdef_u32 b) {       // bits a .. b - 1, b <= 64
    return (b >= 64u ? ~0ull : (1ull << b) - 1ull) & ~((1ull << a) - 1ull);
}

// whole staging words [0, nw) to the room: word k holds the stream's bytes [wbase + 4k, + 4), of
// which those in [0, wl) are written
template <class Io>
WS_DEF_FN void ws_def_flush(Io& io, const wsdef_u32* stg, wsdef_u32 nw, long long wbase, wsdef_u64 wl) {
    for (wsdef_u32 k = io.lane(); k < nw; k += io.lanes()) {
        const long long q = wbase + 4ll * k;
        const wsdef_u32 v = stg[k];
        if (q >= 0 && (wsdef_u64)q + 4 <= wl) {
            io.out_word((wsdef_u64)q, v);
        } else {
            for (wsdef_u32 b = 0; b < 4; ++b)
                if (q + b >= 0 && (wsdef_u64)(q + b) < wl) io.out_byte((wsdef_u64)(q + b), (v >> (8u * b)) & 0xFFu);
        }
    }
}

// Compress one message: body bytes [0, len) through io.ld8 / io.ld32, the room's bytes [0, cap)
// through io.out_word / io.out_byte / io.copy. W: scratch. Returns the status; *out_len what the
// room holds, *enc_len the encoded length (0 for a message that is not encoded).
template <class Io>
WS_DEF_FN wsdef_u32 ws_deflate_message(Io& io, wsdef_u64 len, wsdef_u64 cap, wsdef_u64 min_len, WsDefWork* W, wsdef_u64* out_len,
                                       wsdef_u64* enc_len) {
    *out_len = 0;
    *enc_len = 0;
    if (len == 0 || len < min_len) {
        if (len > cap) return WEBSOCKET_DEFLATE_ERR_OUT_SPACE;
        io.copy(len);
        *out_len = len;
        return WEBSOCKET_DEFLATE_PLAIN;
    }
    wsdef_u32* const tab = W->tab;
    wsdef_u32* const stg = W->stg;
    const wsdef_u32 hbits = ws_def_hbits(len), ph = io.phase();
    const wsdef_u64 wl = cap < len - 1 ? cap : len - 1;        // a DEFLATED body has fewer than len bytes: no other byte is needed
    for (wsdef_u32 k = io.lane(); k < (1u << hbits); k += io.lanes()) io.put32(tab + k, WS_DEF_EMPTY);
    for (wsdef_u32 k = io.lane(); k < WS_DEF_STAGE; k += io.lanes()) io.put32(stg + k, k ? 0u : 2u << (8u * ph));   // BFINAL 0, BTYPE 01
    io.sync();
    long long wbase = -(long long)ph;                          // the stream byte staging word 0 starts at
    wsdef_u32 fill = 8u * ph + 3u;                             // bits in the staging buffer
    wsdef_u32 skip = 0;                                        // positions of the next group the last match covers
    for (wsdef_u64 base = 0; base < len; base += WS_DEF_GROUP) {
        const wsdef_u32 n = len - base < WS_DEF_GROUP ? (wsdef_u32)(len - base) : WS_DEF_GROUP;
        const bool look = skip < n;
        wsdef_u32 byte[Io::NL], h[Io::NL], ml[Io::NL], ds[Io::NL], bits[Io::NL], nb[Io::NL], off[Io::NL];
        bool has4[Io::NL], found[Io::NL];
        for (wsdef_u32 l = io.l0(); l < io.l1(); ++l) {
            const wsdef_u32 i = l - io.l0();
            const wsdef_u64 p = base + l;
            has4[i] = l < n && p + 4 <= len;
            const wsdef_u32 w = has4[i] ? io.ld32(p) : (l < n ? io.ld8(p) : 0u);
            byte[i] = w & 0xFFu;
            h[i] = has4[i] ? ws_def_hash(w, hbits) : 0u;
            ml[i] = 0;
            ds[i] = 0;
            if (has4[i] && look && l >= skip) {
                const wsdef_u32 d = (wsdef_u32)p - tab[h[i]];
                if (d >= 1u && d <= WS_DEF_MAXDIST && d <= p) {
                    const wsdef_u32 maxl = len - p < WS_DEF_MAXMATCH ? (wsdef_u32)(len - p) : WS_DEF_MAXMATCH;
                    wsdef_u32 k = 0;
                    bool differ = false;
                    while (!differ && k + 4 <= maxl) {
                        const wsdef_u32 x = io.ld32(p + k) ^ io.ld32(p - d + k);
                        if (x) {
                            k += (wsdef_u32)__builtin_ctz(x) >> 3;
                            differ = true;
                        } else {
                            k += 4;
                        }
                    }
                    while (!differ && k < maxl && io.ld8(p + k) == io.ld8(p - d + k)) ++k;
                    if (k >= WS_DEF_MINMATCH) {
                        ml[i] = k;
                        ds[i] = d;
                    }
                }
            }
            found[i] = ml[i] != 0;
        }
        io.sync();                                             // every lookup reads the table as it stood before the group
        for (wsdef_u32 l = io.l0(); l < io.l1(); ++l)
            if (has4[l - io.l0()]) io.put32(tab + h[l - io.l0()], (wsdef_u32)(base + l));
        io.sync();
        for (wsdef_u32 l = io.l0(); l < io.l1(); ++l)         // the highest position wins (a group never straddles 2^32)
            if (has4[l - io.l0()]) io.max32(tab + h[l - io.l0()], (wsdef_u32)(base + l));
        io.sync();
        if (!look) {
            skip -= n;
            continue;
        }
        const wsdef_u64 M = io.ballot(found);
        wsdef_u64 S = 0;                                       // the positions that start a token
        wsdef_u32 cur = skip;
        while (cur < n) {
            const wsdef_u64 m = M & (~0ull << cur);
            if (!m) {
                S |= ws_def_range(cur, n);
                cur = n;
                break;
            }
            const wsdef_u32 j = io.uni((wsdef_u32)__builtin_ctzll(m));
            S |= ws_def_range(cur, j + 1u);
            cur = j + io.bcast(ml, j);
        }
        skip = cur - n;
        for (wsdef_u32 l = io.l0(); l < io.l1(); ++l) {
            const wsdef_u32 i = l - io.l0();
            bits[i] = 0;
            nb[i] = 0;
            if ((S >> l) & 1ull) nb[i] = ml[i] ? ws_def_match(ml[i], ds[i], &bits[i]) : ws_def_literal(byte[i], &bits[i]);
        }
        const wsdef_u32 total = io.scan(nb, off);
        for (wsdef_u32 l = io.l0(); l < io.l1(); ++l) {
            const wsdef_u32 i = l - io.l0();
            if (nb[i]) {
                const wsdef_u32 at = fill + off[i], sh = at & 31u;
                io.or32(stg + (at >> 5), bits[i] << sh);
                if (sh + nb[i] > 32u) io.or32(stg + (at >> 5) + 1, bits[i] >> (32u - sh));
            }
        }
        fill += total;
        io.sync();
        const wsdef_u32 nw = fill >> 5;
        if (nw) {
            ws_def_flush(io, stg, nw, wbase, wl);
            const wsdef_u32 carry = io.uni(stg[nw]);
            io.sync();
            for (wsdef_u32 k = io.lane(); k <= nw; k += io.lanes()) io.put32(stg + k, k ? 0u : carry);
            io.sync();
            wbase += 4ll * nw;
            fill &= 31u;
        }
    }
    fill += 10u;                                               // end of block (7 zero bits), an empty stored block's 000
    const wsdef_u32 nbytes = (fill + 7u) >> 3;
    for (wsdef_u32 k = io.lane(); k < nbytes; k += io.lanes()) {
        const long long q = wbase + (long long)k;
        if (q >= 0 && (wsdef_u64)q < wl) io.out_byte((wsdef_u64)q, (stg[k >> 2] >> (8u * (k & 3u))) & 0xFFu);
    }
    const wsdef_u64 enc = (wsdef_u64)(wbase + (long long)nbytes);
    *enc_len = enc;
    if (enc < len && enc <= cap) {
        *out_len = enc;
        return WEBSOCKET_DEFLATE_DEFLATED;
    }
    if (len > cap) return WEBSOCKET_DEFLATE_ERR_OUT_SPACE;
    io.sync();
    io.copy(len);
    *out_len = len;
    return WEBSOCKET_DEFLATE_PLAIN;
}

// One entry of a list, written against a Slot: deflate(m, off, cap, min_len, &out_len) runs
// ws_deflate_message on the entry's body with the room at off (counted from the destination base).
template <class Slot>
WS_DEF_FN WebsocketDeflateMsgRes_t ws_deflate_entry(Slot& c, const WebsocketDeflateMsg_t& m, wsdef_u64 src_len, wsdef_u64 min_len,
                                                    wsdef_u64 off, wsdef_u64 cap) {
    WebsocketDeflateMsgRes_t r;
    r.out_off = off;
    r.out_len = 0;
    r.reserved = 0;
    if (m.type == WEBSOCKET_SEND_SKIP) r.status = WEBSOCKET_DEFLATE_SKIPPED;
    else if (m.len > src_len || m.src_off > src_len - m.len) r.status = WEBSOCKET_DEFLATE_ERR_RANGE;
    else r.status = c.deflate(m, off, cap, min_len, &r.out_len);
    return r;
}

// what the send list takes from an entry and its result (websocketframeBatchSendListFromDeflatedDevice)
WS_DEF_FN WebsocketSendMsg_t ws_deflate_send_entry(wsdef_u32 type, const WebsocketDeflateMsgRes_t& r) {
    WebsocketSendMsg_t o;
    const bool sent = type != WEBSOCKET_SEND_SKIP && (r.status == WEBSOCKET_DEFLATE_DEFLATED || r.status == WEBSOCKET_DEFLATE_PLAIN);
    o.src_off = sent ? r.out_off : 0ull;
    o.len = sent ? r.out_len : 0ull;
    o.type = !sent ? WEBSOCKET_SEND_SKIP : (r.status == WEBSOCKET_DEFLATE_DEFLATED ? type | WEBSOCKET_SEND_TYPE_RSV1 : type);
    o.reserved = 0;
    return o;
}

// ---- the host's Io and Slot: every loop whole, plain memory
struct WsDefHostIo {
    static const wsdef_u32 NL = WS_DEF_GROUP;
    const unsigned char* src;            // the message's body
    unsigned char* dst;                  // the room's first byte
    wsdef_u32 l0() const { return 0; }
    wsdef_u32 l1() const { return WS_DEF_GROUP; }
    wsdef_u32 lane() const { return 0; }
    wsdef_u32 lanes() const { return 1; }
    wsdef_u32 uni(wsdef_u32 v) const { return v; }
    void sync() {}
    wsdef_u32 phase() const { return (wsdef_u32)((uintptr_t)dst & 3u); }
    wsdef_u32 ld8(wsdef_u64 i) const { return src[i]; }
    wsdef_u32 ld32(wsdef_u64 i) const {
        return (wsdef_u32)src[i] | (wsdef_u32)src[i + 1] << 8 | (wsdef_u32)src[i + 2] << 16 | (wsdef_u32)src[i + 3] << 24;
    }
    void put32(wsdef_u32* p, wsdef_u32 v) { *p = v; }
    void max32(wsdef_u32* p, wsdef_u32 v) { if (*p < v) *p = v; }
    void or32(wsdef_u32* p, wsdef_u32 v) { *p |= v; }
    wsdef_u64 ballot(const bool* f) const {
        wsdef_u64 m = 0;
        for (wsdef_u32 l = 0; l < WS_DEF_GROUP; ++l) m |= (wsdef_u64)(f[l] ? 1u : 0u) << l;
        return m;
    }
    wsdef_u32 bcast(const wsdef_u32* v, wsdef_u32 j) const { return v[j]; }
    wsdef_u32 scan(const wsdef_u32* v, wsdef_u32* excl) const {
        wsdef_u32 s = 0;
        for (wsdef_u32 l = 0; l < WS_DEF_GROUP; ++l) {
            excl[l] = s;
            s += v[l];
        }
        return s;
    }
    void out_word(wsdef_u64 q, wsdef_u32 v) {
        for (wsdef_u32 b = 0; b < 4; ++b) dst[q + b] = (unsigned char)(v >> (8u * b));
    }
    void out_byte(wsdef_u64 q, wsdef_u32 v) { dst[q] = (unsigned char)v; }
    void copy(wsdef_u64 n) {
        for (wsdef_u64 k = 0; k < n; ++k) dst[k] = src[k];
    }
};

struct WsDefHostSlot {
    const unsigned char* src;
    unsigned char* dst;
    WsDefWork W;
    wsdef_u64 enc_len;                   // of the last entry that ran
    wsdef_u32 deflate(const WebsocketDeflateMsg_t& m, wsdef_u64 off, wsdef_u64 cap, wsdef_u64 min_len, wsdef_u64* out_len) {
        WsDefHostIo io;
        io.src = src + m.src_off;
        io.dst = dst + off;
        return ws_deflate_message(io, m.len, cap, min_len, &W, out_len, &enc_len);
    }
};

// one connection's list on the host; enc_len (may be NULL): every entry's encoded length.
// Returns the entries that ended DEFLATED or PLAIN.
static inline wsdef_u64 ws_deflate_list(const unsigned char* src, wsdef_u64 src_len, const WebsocketDeflateMsg_t* msg, wsdef_u32 nmsg,
                                        wsdef_u64 min_len, unsigned char* dst, const wsdef_u64* dst_off, const wsdef_u64* dst_cap,
                                        WebsocketDeflateMsgRes_t* msg_res, wsdef_u64* enc_len) {
    WsDefHostSlot c;
    c.src = src;
    c.dst = dst;
    wsdef_u64 sent = 0;
    for (wsdef_u32 i = 0; i < nmsg; ++i) {
        c.enc_len = 0;
        msg_res[i] = ws_deflate_entry(c, msg[i], src_len, min_len, dst_off[i], dst_cap[i]);
        if (enc_len) enc_len[i] = c.enc_len;
        if (msg_res[i].status == WEBSOCKET_DEFLATE_DEFLATED || msg_res[i].status == WEBSOCKET_DEFLATE_PLAIN) ++sent;
    }
    return sent;
}
