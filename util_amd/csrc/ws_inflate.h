// ws_inflate.h — the rule of websocketframeBatchInflateDevice and websocketframeInflateHost
// (include/wsframe_amd_deflate.h), defined once: raw DEFLATE (RFC 1951) over a message body
// followed by the four virtual bytes 00 00 FF FF (RFC 7692 section 7.2.2), judged where zlib's
// inflate judges, and the walk over a connection's list (first failure, NOT_RUN, the packing of the
// outputs). Plain C++ — no HIP header, no AMDGPU builtin — so the kernel (ws_inflate.hip), the host
// entry point and a CPU test (tests/test_inflate_host.py) compile the same text.
//
// The decoder is written against an Io: where body bytes come from, where output bytes go, how a
// table word is stored, which share of a table fill is this caller's, and uni(): a value every
// caller of the group holds alike (the kernel makes it a scalar). On the host an Io is two
// pointers and every loop runs whole; in the kernel one wavefront runs the decoder with every value
// wave-uniform, one lane stores table words, the 64 lanes share the lookup fill, and a literal run,
// a match or a stored block is one cooperative copy.
//
// Tables (WsInfTabs, 1,856 B per set): a first-level lookup of 9 bits (literal/length) and 6 bits
// (distance), entry = code length << 12 | symbol, and puff's canonical count / symbol arrays for the
// longer codes, which are decoded a bit at a time. The code-length code (19 symbols, at most 7
// bits) has no lookup. Base values and extra bits of lengths and distances are computed, not tabled.
#pragma once
#include <stdint.h>

#include "../../include/wsframe_amd_deflate.h"

#ifdef __HIPCC__
#define WS_INF_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define WS_INF_FN static inline
#endif

typedef unsigned long long wsinf_u64;
typedef unsigned int wsinf_u32;
typedef unsigned short wsinf_u16;
typedef unsigned char wsinf_u8;

#define WS_INF_LBITS 9u
#define WS_INF_DBITS 6u
#define WS_INF_LONG 0xFFFFu          // lookup entry: the code is longer than the lookup
#define WS_INF_BADSYM 0xFFFu         // lookup entry's symbol: no such code (1 bit, as zlib's filler entries)
#define WS_INF_MAXBITS 15u

struct WsInfTabs {                   // one block's (or the fixed) pair of codes
    wsinf_u16 llook[1u << WS_INF_LBITS], lcount[16], lsym[288];
    wsinf_u16 dlook[1u << WS_INF_DBITS], dcount[16], dsym[32];
};
struct WsInfWork {                   // what a dynamic header needs while it is read
    wsinf_u8 lens[320];              // the code lengths, literal/length then distance (286 + 30)
    wsinf_u16 offs[16], ccount[16], csym[20];
};

// zlib's inflate_table verdict over n code lengths, and puff's construction: count[len], and the
// symbols sorted by (length, symbol). `codes`: the code-length code, which may not be incomplete at
// all. Returns 0 ok, 1 ok and empty (no symbol has a code: every code is then bad and one bit
// long; for the code-length code zlib reads such a bit as symbol 0), -1 error. With lbits > 0 the
// lookup is filled too; the caller syncs before it reads the tables.
template <class Io>
WS_INF_FN int ws_inf_build(Io& io, const wsinf_u8* lens, wsinf_u32 n, bool codes, wsinf_u32 lbits, wsinf_u16* look, wsinf_u16* count,
                           wsinf_u16* sym, wsinf_u16* offs) {
    for (wsinf_u32 l = 0; l <= WS_INF_MAXBITS; ++l) io.st16(count + l, 0);
    io.sync();
    for (wsinf_u32 s = 0; s < n; ++s) {
        const wsinf_u32 l = io.uni(lens[s]);
        io.st16(count + l, (wsinf_u16)(io.uni(count[l]) + 1u));
        io.sync();
    }
    const bool empty = io.uni(count[0]) == n;
    int left = 1;
    wsinf_u32 maxl = 0;
    for (wsinf_u32 l = 1; l <= WS_INF_MAXBITS; ++l) {
        const wsinf_u32 c = io.uni(count[l]);
        if (c) maxl = l;
        left = (left << 1) - (int)c;
        if (left < 0 && !empty) return -1;                         // over-subscribed
    }
    const bool incomplete = !empty && left > 0;
    if (incomplete && (codes || maxl != 1)) return -1;
    io.st16(offs + 0, 0);
    io.st16(offs + 1, 0);
    io.sync();
    for (wsinf_u32 l = 1; l < WS_INF_MAXBITS; ++l) {
        io.st16(offs + l + 1, (wsinf_u16)(io.uni(offs[l]) + io.uni(count[l])));
        io.sync();
    }
    for (wsinf_u32 s = 0; s < n; ++s) {
        const wsinf_u32 l = io.uni(lens[s]);
        if (l) {
            const wsinf_u32 at = io.uni(offs[l]);
            io.st16(sym + at, (wsinf_u16)s);
            io.st16(offs + l, (wsinf_u16)(at + 1u));
            io.sync();
        }
    }
    if (lbits) {
        const wsinf_u32 size = 1u << lbits, nsym = n - io.uni(count[0]);
        const wsinf_u16 fill = (empty || incomplete) ? (wsinf_u16)(1u << 12 | WS_INF_BADSYM) : (wsinf_u16)WS_INF_LONG;
        for (wsinf_u32 k = io.lane(); k < size; k += io.lanes()) io.put16(look + k, fill);
        io.sync();
        // sorted position j -> its length and canonical code; the code, bit-reversed, at every
        // lookup index that ends in it
        for (wsinf_u32 j = io.lane(); j < nsym; j += io.lanes()) {
            wsinf_u32 first = 0, start = 0;
            for (wsinf_u32 l = 1; l <= lbits; ++l) {
                const wsinf_u32 c = count[l];
                if (j < start + c) {
                    const wsinf_u32 code = first + (j - start);
                    wsinf_u32 rev = 0;
                    for (wsinf_u32 b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1u - b);
                    const wsinf_u16 e = (wsinf_u16)(l << 12 | sym[j]);
                    for (wsinf_u32 k = rev; k < size; k += 1u << l) io.put16(look + k, e);
                    break;
                }
                first = (first + c) << 1;
                start += c;
            }
        }
    }
    return empty ? 1 : 0;
}

// One symbol of a code from the low bits of `hold`, of which nbits are real (the rest zero).
// Returns its length (> 0, *out the symbol), 0 when the input holds no whole code, -1 for a code
// that is not in the (incomplete) set.
template <class Io>
WS_INF_FN int ws_inf_symbol(Io& io, wsinf_u64 hold, wsinf_u32 nbits, const wsinf_u16* look, wsinf_u32 lbits, const wsinf_u16* count,
                            const wsinf_u16* sym, wsinf_u32* out) {
    if (lbits) {
        const wsinf_u32 e = io.uni(look[(wsinf_u32)hold & ((1u << lbits) - 1u)]);
        if (e != WS_INF_LONG) {
            const wsinf_u32 l = e >> 12;
            if (l > nbits) return 0;
            *out = e & 0xFFFu;
            return (e & 0xFFFu) == WS_INF_BADSYM ? -1 : (int)l;
        }
    }
    int code = 0, first = 0, index = 0;
    for (wsinf_u32 l = 1; l <= WS_INF_MAXBITS; ++l) {
        if (l > nbits) return 0;
        code |= (int)((hold >> (l - 1u)) & 1u);
        const int c = (int)io.uni(count[l]);
        if (code - c < first) {
            *out = io.uni(sym[index + (code - first)]);
            return (int)l;
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// the fixed code of RFC 1951 section 3.2.6 (288 and 32 symbols: the four that never occur keep their
// codes and are judged when they are decoded)
template <class Io>
WS_INF_FN void ws_inf_build_fixed(Io& io, WsInfTabs* T, WsInfWork* W) {
    for (wsinf_u32 s = io.lane(); s < 288; s += io.lanes()) io.put8(W->lens + s, (wsinf_u8)(s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8))));
    io.sync();
    ws_inf_build(io, W->lens, 288, false, WS_INF_LBITS, T->llook, T->lcount, T->lsym, W->offs);
    io.sync();
    for (wsinf_u32 s = io.lane(); s < 32; s += io.lanes()) io.put8(W->lens + s, 5);
    io.sync();
    ws_inf_build(io, W->lens, 32, false, WS_INF_DBITS, T->dlook, T->dcount, T->dsym, W->offs);
    io.sync();
}

struct WsInfBits {                   // the bit reader: `hold` has nbits real bits, `at` is the next input byte
    wsinf_u64 hold, at, total;             // total = body length + 4
    wsinf_u32 nbits;
};

template <class Io>
WS_INF_FN void ws_inf_refill(Io& io, WsInfBits& b, wsinf_u64 len) {
    while (b.nbits <= 56 && b.at < b.total) {
        // the virtual tail 00 00 FF FF behind the body
        const wsinf_u32 v = b.at < len ? io.in_byte(b.at) : (b.at - len < 2 ? 0u : 0xFFu);
        b.hold |= (wsinf_u64)v << b.nbits;
        b.nbits += 8;
        ++b.at;
    }
}
WS_INF_FN wsinf_u32 ws_inf_take(WsInfBits& b, wsinf_u32 n) {
    const wsinf_u32 v = (wsinf_u32)(b.hold & ((1ull << n) - 1ull));
    b.hold >>= n;
    b.nbits -= n;
    return v;
}

// where a message's next n output bytes stand against its limits: 0 write them, 1 count them only
// (they do not fit the room: the message goes on unwritten), 2 stop. zlib is given room for
// max_message_size + 1 bytes and stops at the first symbol that needs a byte more; until then it
// goes on judging, so an error right behind byte max_message_size + 1 still counts, and a message
// that ends with that byte is too big.
struct WsInfOut {
    wsinf_u64 pos, limit, room;            // bytes so far; max_message_size (0: none); what the connection has left
    bool dry;
};
WS_INF_FN wsinf_u32 ws_inf_room(WsInfOut& o, wsinf_u64 n) {
    if (o.limit && n && o.pos + n - 1 > o.limit) return 2;
    if (o.pos + n > o.room) o.dry = true;
    return o.dry ? 1u : 0u;
}

// Inflate one message: body bytes [0, len) through io.in_byte, output through io.lit / io.match /
// io.stored (positions count from the message's first output byte). T: the block's tables, F: the
// fixed tables (built once by the caller), W: header scratch. Returns the status; *out_len the
// message's length when it is WEBSOCKET_INFLATE_OK.
template <class Io>
WS_INF_FN wsinf_u32 ws_inflate_message(Io& io, wsinf_u64 len, wsinf_u64 limit, wsinf_u64 room, WsInfTabs* T, const WsInfTabs* F, WsInfWork* W,
                                 wsinf_u64* out_len) {
    WsInfBits b;
    b.hold = 0; b.at = 0; b.total = len + 4; b.nbits = 0;
    WsInfOut o;
    o.pos = 0; o.limit = limit; o.room = room; o.dry = false;
    *out_len = 0;
    for (;;) {
        ws_inf_refill(io, b, len);
        if (b.nbits < 3) break;
        const wsinf_u32 bfinal = ws_inf_take(b, 1), type = ws_inf_take(b, 2);
        const WsInfTabs* C = F;
        if (type == 3) return WEBSOCKET_INFLATE_ERR_DATA;
        if (type == 0) {
            ws_inf_take(b, b.nbits & 7u);
            if (b.nbits < 32) break;
            const wsinf_u32 v = ws_inf_take(b, 32);
            if ((v & 0xFFFFu) != ((v >> 16) ^ 0xFFFFu)) return WEBSOCKET_INFLATE_ERR_DATA;
            // the bytes still in the bit buffer go back to the input
            b.at -= b.nbits >> 3;
            b.hold = 0;
            b.nbits = 0;
            const wsinf_u64 have = b.total - b.at;
            const wsinf_u32 want = v & 0xFFFFu, n = have < want ? (wsinf_u32)have : want;
            const wsinf_u32 r = ws_inf_room(o, n);
            if (r == 2) return WEBSOCKET_INFLATE_ERR_TOO_BIG;
            if (n) {
                // body bytes as one copy, tail bytes as literals
                const wsinf_u32 nb = b.at < len ? (len - b.at < n ? (wsinf_u32)(len - b.at) : n) : 0u;
                if (r == 0) {
                    if (nb) io.stored(o.pos, b.at, nb);
                    for (wsinf_u32 k = nb; k < n; ++k) io.lit(o.pos + k, b.at + k - len < 2 ? 0u : 0xFFu);
                }
                o.pos += n;
                b.at += n;
            }
            if (n < want) break;
            if (bfinal) break;
            continue;
        }
        if (type == 2) {
            if (b.nbits < 14) break;
            const wsinf_u32 nlen = ws_inf_take(b, 5) + 257, ndist = ws_inf_take(b, 5) + 1, ncode = ws_inf_take(b, 4) + 4;
            if (nlen > 286 || ndist > 30) return WEBSOCKET_INFLATE_ERR_DATA;
            for (wsinf_u32 k = io.lane(); k < 19; k += io.lanes()) io.put8(W->lens + k, 0);
            io.sync();
            bool out_of_input = false;
            for (wsinf_u32 k = 0; k < ncode; ++k) {
                ws_inf_refill(io, b, len);
                if (b.nbits < 3) { out_of_input = true; break; }
                // the order of RFC 1951 section 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                const wsinf_u32 pos = k < 3 ? 16 + k : (k == 3 ? 0u : ((k & 1u) ? 8u - ((k - 3u) >> 1) : 7u + ((k - 2u) >> 1)));
                io.st8(W->lens + pos, (wsinf_u8)ws_inf_take(b, 3));
            }
            if (out_of_input) break;
            io.sync();
            const int cb = ws_inf_build(io, W->lens, 19, true, 0, (wsinf_u16*)0, W->ccount, W->csym, W->offs);
            if (cb < 0) return WEBSOCKET_INFLATE_ERR_DATA;
            io.sync();
            wsinf_u32 idx = 0;
            while (idx < nlen + ndist) {
                ws_inf_refill(io, b, len);
                wsinf_u32 s = 0;
                int l = 1;
                if (cb == 1) {
                    if (b.nbits < 1) l = 0;
                } else {
                    l = ws_inf_symbol(io, b.hold, b.nbits, (const wsinf_u16*)0, 0, W->ccount, W->csym, &s);
                }
                if (l == 0) { out_of_input = true; break; }
                if (l < 0) return WEBSOCKET_INFLATE_ERR_DATA;
                if (s < 16) {
                    ws_inf_take(b, (wsinf_u32)l);
                    io.st8(W->lens + idx, (wsinf_u8)s);
                    ++idx;
                    continue;
                }
                const wsinf_u32 xb = s == 16 ? 2u : (s == 17 ? 3u : 7u);
                if (b.nbits < (wsinf_u32)l + xb) { out_of_input = true; break; }
                ws_inf_take(b, (wsinf_u32)l);
                wsinf_u32 prev = 0;
                if (s == 16) {
                    if (idx == 0) return WEBSOCKET_INFLATE_ERR_DATA;
                    io.sync();
                    prev = io.uni(W->lens[idx - 1]);
                }
                const wsinf_u32 rep = (s == 18 ? 11u : 3u) + ws_inf_take(b, xb);
                if (idx + rep > nlen + ndist) return WEBSOCKET_INFLATE_ERR_DATA;
                for (wsinf_u32 k = 0; k < rep; ++k) io.st8(W->lens + idx + k, (wsinf_u8)prev);
                idx += rep;
            }
            if (out_of_input) break;
            io.sync();
            if (io.uni(W->lens[256]) == 0) return WEBSOCKET_INFLATE_ERR_DATA;
            if (ws_inf_build(io, W->lens, nlen, false, WS_INF_LBITS, T->llook, T->lcount, T->lsym, W->offs) < 0)
                return WEBSOCKET_INFLATE_ERR_DATA;
            io.sync();
            if (ws_inf_build(io, W->lens + nlen, ndist, false, WS_INF_DBITS, T->dlook, T->dcount, T->dsym, W->offs) < 0)
                return WEBSOCKET_INFLATE_ERR_DATA;
            io.sync();
            C = T;
        }
        // the block's symbols
        bool ended = false;
        for (;;) {
            ws_inf_refill(io, b, len);
            wsinf_u32 s = 0;
            int l = ws_inf_symbol(io, b.hold, b.nbits, C->llook, WS_INF_LBITS, C->lcount, C->lsym, &s);
            if (l == 0) { ended = true; break; }
            if (l < 0) return WEBSOCKET_INFLATE_ERR_DATA;
            ws_inf_take(b, (wsinf_u32)l);
            if (s < 256) {
                const wsinf_u32 r = ws_inf_room(o, 1);
                if (r == 2) return WEBSOCKET_INFLATE_ERR_TOO_BIG;
                if (r == 0) io.lit(o.pos, s);
                ++o.pos;
                continue;
            }
            if (s == 256) break;
            if (s >= 286) return WEBSOCKET_INFLATE_ERR_DATA;
            // length s - 257: 3..10 plain, then four per extra-bit count, 258 for the last
            const wsinf_u32 i = s - 257, le = i < 8 || i == 28 ? 0u : (i >> 2) - 1u;
            wsinf_u32 mlen = i < 8 ? 3 + i : (i == 28 ? 258u : 3u + ((4u + (i & 3u)) << le));
            if (b.nbits < le) { ended = true; break; }
            mlen += ws_inf_take(b, le);
            wsinf_u32 d = 0;
            l = ws_inf_symbol(io, b.hold, b.nbits, C->dlook, WS_INF_DBITS, C->dcount, C->dsym, &d);
            if (l == 0) { ended = true; break; }
            if (l < 0 || d >= 30) return WEBSOCKET_INFLATE_ERR_DATA;
            ws_inf_take(b, (wsinf_u32)l);
            const wsinf_u32 de = d < 4 ? 0u : (d >> 1) - 1u;
            wsinf_u32 dist = d < 4 ? 1 + d : 1u + ((2u + (d & 1u)) << de);
            if (b.nbits < de) { ended = true; break; }
            dist += ws_inf_take(b, de);
            if (o.limit && o.pos > o.limit) return WEBSOCKET_INFLATE_ERR_TOO_BIG;   // (zlib: no room left comes first)
            if (dist > o.pos) return WEBSOCKET_INFLATE_ERR_DATA;
            const wsinf_u32 r = ws_inf_room(o, mlen);
            if (r == 2) return WEBSOCKET_INFLATE_ERR_TOO_BIG;
            if (r == 0) io.match(o.pos, dist, mlen);
            o.pos += mlen;
        }
        if (ended || bfinal) break;
    }
    if (o.limit && o.pos > o.limit) return WEBSOCKET_INFLATE_ERR_TOO_BIG;
    if (o.dry) return WEBSOCKET_INFLATE_ERR_OUT_SPACE;
    *out_len = o.pos;
    return WEBSOCKET_INFLATE_OK;
}

WS_INF_FN wsinf_u32 ws_inflate_close_status(wsinf_u32 status) {
    return status == WEBSOCKET_INFLATE_ERR_DATA ? 1007u : (status == WEBSOCKET_INFLATE_ERR_TOO_BIG ? 1009u : 0u);
}

// The walk over one connection's list, written against a Conn: entry(i) loads entry i,
// inflate(m, out_off, room, &n) runs ws_inflate_message on it with the connection's output at
// out_off (counted from the destination base), result(i, r) stores a message record. base: the
// room's first byte counted from the destination base, cap: the room.
template <class Conn>
WS_INF_FN WebsocketInflateResult_t ws_inflate_walk(Conn& c, wsinf_u32 n, wsinf_u64 src_len, wsinf_u64 base, wsinf_u64 cap) {
    WebsocketInflateResult_t R;
    R.out_len = 0;
    R.n_msgs = 0;
    R.status = WEBSOCKET_INFLATE_OK;
    R.first_bad = WEBSOCKET_INFLATE_NONE;
    R.close_status = 0;
    for (wsinf_u32 i = 0; i < n; ++i) {
        WebsocketInflateMsgRes_t r;
        r.out_off = base + R.out_len;
        r.out_len = 0;
        r.status = WEBSOCKET_INFLATE_OK;
        r.reserved = 0;
        if (R.status != WEBSOCKET_INFLATE_OK) {
            r.status = WEBSOCKET_INFLATE_NOT_RUN;
            c.result(i, r);
            continue;
        }
        const WebsocketInflateMsg_t m = c.entry(i);
        if (m.kind != WEBSOCKET_INFLATE_SKIP) {
            if (m.kind != WEBSOCKET_INFLATE_RAW || m.src_off > src_len || m.len > src_len - m.src_off) {
                r.status = WEBSOCKET_INFLATE_ERR_RANGE;
            } else {
                wsinf_u64 got = 0;
                r.status = c.inflate(m, r.out_off, cap - R.out_len, &got);
                if (r.status == WEBSOCKET_INFLATE_OK) {
                    r.out_len = got;
                    R.out_len += got;
                    R.n_msgs += 1;
                }
            }
            if (r.status != WEBSOCKET_INFLATE_OK) {
                R.status = r.status;
                R.first_bad = i;
                R.close_status = ws_inflate_close_status(r.status);
            }
        }
        c.result(i, r);
    }
    return R;
}

// ---- the host's Io and Conn: every loop whole, plain memory
struct WsInfHostIo {
    const unsigned char* src;        // the message's body
    unsigned char* dst;              // the message's first output byte
    wsinf_u32 uni(wsinf_u32 v) const { return v; }
    wsinf_u32 lane() const { return 0; }
    wsinf_u32 lanes() const { return 1; }
    void sync() {}
    void st16(wsinf_u16* p, wsinf_u16 v) { *p = v; }
    void put16(wsinf_u16* p, wsinf_u16 v) { *p = v; }
    void st8(wsinf_u8* p, wsinf_u8 v) { *p = v; }
    void put8(wsinf_u8* p, wsinf_u8 v) { *p = v; }
    wsinf_u32 in_byte(wsinf_u64 i) const { return src[i]; }
    void lit(wsinf_u64 pos, wsinf_u32 v) { dst[pos] = (unsigned char)v; }
    void match(wsinf_u64 pos, wsinf_u32 dist, wsinf_u32 n) {
        for (wsinf_u32 k = 0; k < n; ++k) dst[pos + k] = dst[pos - dist + k];
    }
    void stored(wsinf_u64 pos, wsinf_u64 at, wsinf_u32 n) {
        for (wsinf_u32 k = 0; k < n; ++k) dst[pos + k] = src[at + k];
    }
};

struct WsInfHostConn {
    const unsigned char* src;
    const WebsocketInflateMsg_t* msg;
    unsigned char* dst;
    WebsocketInflateMsgRes_t* res;   // may be NULL
    wsinf_u64 limit;
    WsInfTabs T, F;
    WsInfWork W;
    WebsocketInflateMsg_t entry(wsinf_u32 i) const { return msg[i]; }
    void result(wsinf_u32 i, const WebsocketInflateMsgRes_t& r) {
        if (res) res[i] = r;
    }
    wsinf_u32 inflate(const WebsocketInflateMsg_t& m, wsinf_u64 out_off, wsinf_u64 room, wsinf_u64* got) {
        WsInfHostIo io;
        io.src = src + m.src_off;
        io.dst = dst + out_off;
        return ws_inflate_message(io, m.len, limit, room, &T, &F, &W, got);
    }
};

static inline unsigned long long ws_inflate_connection(const unsigned char* src, wsinf_u64 src_len, const WebsocketInflateMsg_t* msg,
                                                       wsinf_u32 nmsg, wsinf_u64 limit, unsigned char* dst, wsinf_u64 dst_cap,
                                                       WebsocketInflateMsgRes_t* msg_res, WebsocketInflateResult_t* out) {
    WsInfHostConn c;
    c.src = src;
    c.msg = msg;
    c.dst = dst;
    c.res = msg_res;
    c.limit = limit;
    WsInfHostIo io;
    io.src = 0;
    io.dst = 0;
    ws_inf_build_fixed(io, &c.F, &c.W);
    *out = ws_inflate_walk(c, nmsg, src_len, 0, dst_cap);
    return out->out_len;
}
