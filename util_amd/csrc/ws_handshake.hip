// ws_handshake.hip — websocketframeBatchHandshakeDevice (include/wsframe_amd_handshake.h): the
// opening handshake of every segment of a device batch, and its host counterpart. The rule is
// ws_handshake.h's; this file only decides who looks at which bytes.
//
//   ws_hs_parse   one wavefront per segment. Rounds of 64 lanes x 16 B, aligned 16-B loads from
//                 the segment's 16-B phase on (chunks that start past the segment's end are not
//                 loaded; the last chunk's over-read stays inside WEBSOCKET_BATCH_PAD). Each lane
//                 tests its 16 positions with three bytes of look-ahead from its neighbour (lane
//                 63 loads them); a ballot finds the round's first terminator and first NUL. The
//                 same sweep verifies the lanes' "Sec-" candidates against the two header names
//                 and keeps the first match of each, so a request is read once; which of them
//                 count is decided when e is known. The value skip and the value end are ballots
//                 over 64 bytes. Lane 0 stores the whole descriptor: the response's length and
//                 flags follow from the parse alone.
//   ws_hs_accept  one lane per segment, so SHA-1's 80 serial rounds run 64 segments wide. Lanes
//                 whose segment has ret <= 0 leave at once. key || GUID is gathered into the
//                 schedule words block by block, the digest becomes 28 characters in 7 dwords,
//                 and the response's fixed part is stored from registers with 16-B stores where
//                 the slot is 16-B aligned, dword stores where it is 4-B aligned and byte stores
//                 otherwise; an echoed protocol range is copied byte by byte. Not launched when
//                 neither accept nor response is asked for.
// No workspace, no host synchronisation: two launches on the caller's stream.
#include <stdio.h>

#include "ws_common.h"
#include "ws_handshake.h"

#define HS_PARSE_T 256          // 4 segments per block
#define HS_ACCEPT_T 64
#define HS_ROUND 1024u          // bytes per round: 64 lanes x 16 B

__device__ __forceinline__ u32 hs_byte(uintptr_t a) { return *gptr<unsigned char>(reinterpret_cast<const void*>(a)); }

// The value after the pattern of m bytes at k (ws_hs_value_seq, 64 bytes per step): false when
// the skip reaches e. Wave-uniform arguments and results.
__device__ __forceinline__ bool hs_value(uintptr_t base, u32 k, u32 m, u32 e, u32 lane, u32& off, u32& len) {
    u32 p = k + m;
    for (;;) {
        if (p >= e) return false;
        const u32 q = p + lane;
        const u64 b = __ballot(q < e && !ws_hs_skips((unsigned char)hs_byte(base + q)));
        if (b) { p += (u32)__builtin_ctzll(b); break; }
        p += 64;
    }
    off = p;
    for (u32 r = p; r <= e; r += 64) {              // base[e] is '\r'
        const u32 q = r + lane;
        const u64 b = __ballot(q <= e && ws_hs_ends((unsigned char)hs_byte(base + q)));
        if (b) { len = r + (u32)__builtin_ctzll(b) - p; return true; }
    }
    return false;
}

__device__ __forceinline__ void hs_store_desc(WebsocketHandshakeDesc_t* out, const WebsocketHandshakeDesc_t& d) {
    u32x4 a, b;
    a.x = (u32)d.ret; a.y = d.key_off; a.z = d.key_len; a.w = d.proto_off;
    b.x = d.proto_len; b.y = d.resp_len; b.z = d.flags; b.w = d.reserved;
    gu32x4* const g = gptr<u32x4>(out);
    g[0] = a;
    g[1] = b;
}

__global__ __launch_bounds__(HS_PARSE_T) void ws_hs_parse(const unsigned char* buf, u64 buflen, const u64* seg_off,
                                                          const u64* seg_len, u32 nseg, u32 flags, u32 has_resp,
                                                          u32 resp_cap, WebsocketHandshakeDesc_t* hs) {
    const u32 lane = threadIdx.x & 63u;
    const u32 s = blockIdx.x * (HS_PARSE_T / 64) + (threadIdx.x >> 6);
    if (s >= nseg) return;                                           // wave-uniform
    const u64 so = seg_off[s], sl = seg_len[s];
    if (sl >= WS_HS_MAX_SEG || so > buflen || sl > buflen - so) {    // never read
        if (lane == 0) hs_store_desc(hs + s, ws_hs_desc_seg_len());
        return;
    }
    const u32 len = (u32)sl;
    const uintptr_t base = reinterpret_cast<uintptr_t>(buf) + so;
    const u32 lead = (u32)(base & 15u);
    const uintptr_t a0 = base - lead;
    const u64 span = (u64)lead + len;                                // bytes from a0 to the segment's end
    u32 T = WEBSOCKET_HS_NONE, Z = WEBSOCKET_HS_NONE, K = WEBSOCKET_HS_NONE, P = WEBSOCKET_HS_NONE;
    for (u64 rb = 0; rb < span && T == WEBSOCKET_HS_NONE && Z == WEBSOCKET_HS_NONE; rb += HS_ROUND) {
        const u64 cb = rb + 16u * lane;                              // this lane's chunk, from a0
        u32x4 v = {0u, 0u, 0u, 0u};
        if (cb < span) v = *gptr<u32x4>(reinterpret_cast<const void*>(a0 + cb));
        u32 nx = (u32)__shfl_down((int)v.x, 1);
        if (lane == 63) nx = cb + 16 < span ? *gptr<u32>(reinterpret_cast<const void*>(a0 + cb + 16)) : 0u;
        const long long lo = (long long)lead - (long long)cb, hi = (long long)span - (long long)cb;
        const WsHsChunk c = ws_hs_chunk(v.x, v.y, v.z, v.w, nx, lo, hi, hi - 3);
        // the lanes' candidates against the two header names (a handful per request)
        u32 myk = WEBSOCKET_HS_NONE, myp = WEBSOCKET_HS_NONE;
        for (u32 m = c.sec; m; m &= m - 1) {
            const u32 p = (u32)(cb - lead) + (u32)__builtin_ctz(m);
            const int kind = ws_hs_pattern_at(reinterpret_cast<const unsigned char*>(base + p), len - p);
            if (kind == 1 && myk == WEBSOCKET_HS_NONE) myk = p;
            if (kind == 2 && myp == WEBSOCKET_HS_NONE) myp = p;
        }
        const u64 bk = __ballot(myk != WEBSOCKET_HS_NONE), bp = __ballot(myp != WEBSOCKET_HS_NONE);
        if (K == WEBSOCKET_HS_NONE && bk) K = (u32)__shfl((int)myk, (int)__builtin_ctzll(bk));
        if (P == WEBSOCKET_HS_NONE && bp) P = (u32)__shfl((int)myp, (int)__builtin_ctzll(bp));
        const u64 bt = __ballot(c.term != 0), bz = __ballot(c.nul != 0);
        const u32 pos = (u32)(cb - lead);                            // (wraps where lo > 0: those bits are masked)
        if (bt) T = (u32)__shfl((int)(pos + (c.term ? (u32)__builtin_ctz(c.term) : 0u)), (int)__builtin_ctzll(bt));
        if (bz) Z = (u32)__shfl((int)(pos + (c.nul ? (u32)__builtin_ctz(c.nul) : 0u)), (int)__builtin_ctzll(bz));
    }
    int ret = 0;
    u32 ko = 0, kl = 0, po = WEBSOCKET_HS_NONE, pl = 0;
    if (ws_hs_complete(T, Z)) {
        const u32 e = T;
        ret = -1;
        if (ws_hs_header_counts(K, WS_HS_KEY_PAT_LEN, e) && hs_value(base, K, WS_HS_KEY_PAT_LEN, e, lane, ko, kl)) {
            ret = (int)(e + 4u);
            if (!ws_hs_header_counts(P, WS_HS_PROTO_PAT_LEN, e) || !hs_value(base, P, WS_HS_PROTO_PAT_LEN, e, lane, po, pl)) {
                po = WEBSOCKET_HS_NONE;
                pl = 0;
            }
        }
    }
    if (lane == 0) hs_store_desc(hs + s, ws_hs_desc(ret, ko, kl, po, pl, flags, has_resp != 0, resp_cap));
}

// n fixed bytes (129 or 151) from the registers R to dst: the widest stores dst's address allows
__device__ __forceinline__ void hs_store_fixed(unsigned char* dst, const u32 (&R)[WS_HS_FIXED_WORDS], u32 n) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
    gu8* const g8 = gptr<unsigned char>(dst);
    if ((a & 3u) == 0) {
        if ((a & 15u) == 0) {
            gu32x4* const g16 = gptr<u32x4>(dst);
#pragma unroll
            for (int i = 0; i < 8; ++i) {                            // 128 bytes: both lengths pass them
                u32x4 v;
                v.x = R[4 * i]; v.y = R[4 * i + 1]; v.z = R[4 * i + 2]; v.w = R[4 * i + 3];
                g16[i] = v;
            }
        } else {
            gu32* const g4 = gptr<u32>(dst);
#pragma unroll
            for (int i = 0; i < 32; ++i) g4[i] = R[i];
        }
        gu32* const g4 = gptr<u32>(dst);
#pragma unroll
        for (int i = 32; i < (int)WS_HS_FIXED_WORDS; ++i) {
            if (4u * i + 4u <= n) {
                g4[i] = R[i];
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (4u * i + b < n) g8[4 * i + b] = (unsigned char)(R[i] >> (8 * b));
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < (int)WS_HS_FIXED_WORDS; ++i) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (4u * i + b < n) g8[4 * i + b] = (unsigned char)(R[i] >> (8 * b));
    }
}

__global__ __launch_bounds__(HS_ACCEPT_T) void ws_hs_accept_kernel(const unsigned char* buf, const u64* seg_off, u32 nseg,
                                                                   const WebsocketHandshakeDesc_t* hs,
                                                                   unsigned char* accept, unsigned char* resp,
                                                                   const u64* resp_off, u32 resp_cap) {
    const u32 s = blockIdx.x * HS_ACCEPT_T + threadIdx.x;
    if (s >= nseg) return;
    const gu32x4* const d = gptr<u32x4>(hs + s);
    const u32x4 d0 = d[0], d1 = d[1];
    if ((int)d0.x <= 0) return;
    const bool write = resp && (d1.z & WEBSOCKET_HS_RESP_WRITTEN);
    if (!accept && !write) return;
    const unsigned char* const seg = buf + seg_off[s];
    const u32 key_len = d0.z;
    u32 h[5], w[16], acc[7];
    ws_hs_sha1_init(h);
    const u32 nb = ws_hs_sha1_blocks(key_len);
    for (u32 b = 0; b < nb; ++b) {
        ws_hs_msg_block(seg + d0.y, key_len, nb, b, w);
        ws_hs_sha1_block(h, w);
    }
    ws_hs_accept(h, acc);
    if (accept) {
        gu32x4* const ga = gptr<u32x4>(accept + 32ull * s);
        u32x4 lo4, hi4;
        lo4.x = acc[0]; lo4.y = acc[1]; lo4.z = acc[2]; lo4.w = acc[3];
        hi4.x = acc[4]; hi4.y = acc[5]; hi4.z = acc[6]; hi4.w = 0u;
        ga[0] = lo4;
        ga[1] = hi4;
    }
    if (!write) return;
    const u32 resp_len = d1.y, proto_off = d0.w, proto_len = d1.x;
    const bool wp = resp_len != WS_HS_RESP_PLAIN;
    unsigned char* const dst = resp + (resp_off ? resp_off[s] : (u64)s * resp_cap);
    u32 R[WS_HS_FIXED_WORDS];
#pragma unroll
    for (int i = 0; i < (int)WS_HS_FIXED_WORDS; ++i) R[i] = ws_hs_fixed_word(i, acc, wp);
    const u32 fixed = wp ? WS_HS_FIXED_PROTO : WS_HS_RESP_PLAIN;
    hs_store_fixed(dst, R, fixed);
    if (wp) {
        gu8* const g8 = gptr<unsigned char>(dst + fixed);
        const gu8* const src = gptr<unsigned char>(seg + proto_off);
        for (u32 i = 0; i < proto_len; ++i) g8[i] = src[i];
        g8[proto_len] = '\r'; g8[proto_len + 1] = '\n'; g8[proto_len + 2] = '\r'; g8[proto_len + 3] = '\n';
    }
}

static int hs_flags(const char* who, unsigned int flags) {
    static thread_local char msg[128];
    if (!(flags & ~WEBSOCKET_HS_ECHO_PROTOCOL)) return 0;
    snprintf(msg, sizeof(msg), "%s: unknown flag", who);
    return ws_set_msg(msg);
}

extern "C" WSFRAME_AMD_HS_EXPORT int websocketframeBatchHandshakeDevice(
    const unsigned char* d_buf, unsigned long long buflen, const unsigned long long* d_seg_off,
    const unsigned long long* d_seg_len, unsigned int nseg, unsigned int flags, WebsocketHandshakeDesc_t* d_hs,
    unsigned char* d_accept, unsigned char* d_resp, const unsigned long long* d_resp_off, unsigned int resp_cap,
    void* hip_stream) {
    if (hs_flags("websocketframeBatchHandshakeDevice", flags)) return -1;
    if (nseg == 0) return 0;
    if (!d_buf || !d_seg_off || !d_seg_len || !d_hs)
        return ws_set_msg("websocketframeBatchHandshakeDevice: invalid argument");
    if ((reinterpret_cast<uintptr_t>(d_hs) | reinterpret_cast<uintptr_t>(d_accept)) & 15)
        return ws_set_msg("websocketframeBatchHandshakeDevice: d_hs/d_accept not 16-B aligned");
    if ((reinterpret_cast<uintptr_t>(d_seg_off) | reinterpret_cast<uintptr_t>(d_seg_len) |
         reinterpret_cast<uintptr_t>(d_resp_off)) & 7)
        return ws_set_msg("websocketframeBatchHandshakeDevice: d_seg_off/d_seg_len/d_resp_off not 8-B aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(ws_hs_parse, dim3((nseg + HS_PARSE_T / 64 - 1) / (HS_PARSE_T / 64)), dim3(HS_PARSE_T), 0, st, d_buf,
                       (u64)buflen, d_seg_off, d_seg_len, nseg, flags, d_resp ? 1u : 0u, resp_cap, d_hs);
    if (d_accept || d_resp)
        hipLaunchKernelGGL(ws_hs_accept_kernel, dim3((nseg + HS_ACCEPT_T - 1) / HS_ACCEPT_T), dim3(HS_ACCEPT_T), 0, st,
                           d_buf, d_seg_off, nseg, d_hs, d_accept, d_resp, d_resp_off, resp_cap);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchHandshakeDevice launch", e);
}

extern "C" WSFRAME_AMD_HS_EXPORT int websocketframeHandshakeHost(const unsigned char* buf, unsigned int len,
                                                                 unsigned int flags, WebsocketHandshakeDesc_t* hs,
                                                                 unsigned char accept[32], unsigned char* resp,
                                                                 unsigned int resp_cap) {
    if (hs_flags("websocketframeHandshakeHost", flags)) return -1;
    if (!hs || (!buf && len)) return ws_set_msg("websocketframeHandshakeHost: invalid argument");
    ws_hs_one(buf, len, flags, hs, accept, resp, resp_cap);
    return 0;
}
