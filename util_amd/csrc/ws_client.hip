// ws_client.hip — websocketframeBatchClientRequestDevice and websocketframeBatchClientVerifyDevice
// (include/wsframe_amd_client.h): the client side of the opening handshake for every connection of
// a device batch, and the two host counterparts. The rule is ws_client.h's; this file only
// decides who looks at which bytes.
//
//   ws_cl_verify   one wavefront per segment, the server parse's shape: rounds of 64 lanes x 16 B,
//                  aligned 16-B loads from the segment's 16-B phase on (chunks that start past the
//                  head's end are not loaded; the last chunk's over-read stays inside
//                  WEBSOCKET_BATCH_PAD). Each lane tests its 16 positions with a look-ahead dword
//                  from its neighbour (lane 63 loads it): terminator starts, line ends, and line
//                  ends after which a 'u', 'c' or 's' begins a line. Ballots give the round's first
//                  terminator and the response's first line end. A lane loads its candidates' name
//                  bytes (all before any compare) and keeps up to two matches: two of the five
//                  names cannot start closer than 10 bytes. The wave then takes the round's
//                  matched headers in position order, each with ballots over 64 bytes per step: the
//                  value's line end and its first and last byte that is not SP or HT, then the
//                  compare (9, 28 bytes) or the element walk of a Connection value, one element per
//                  step. A response is read once; the status line's 13 bytes and, where one
//                  protocol header came, the offered list are looked at when e is known. Lane 0
//                  stores the descriptor.
//   ws_cl_request  one lane per connection, 64 per block, so SHA-1's two blocks run 64 connections
//                  wide from registers (the key's 24 characters are computed, never stored and
//                  re-read). The request's bytes go through a 16-byte funnel in four registers and
//                  leave as 16-B stores; the slot's first and last chunk store exactly their own
//                  bytes (dword stores for whole dwords, byte stores inside partial ones), so
//                  slots may lie anywhere and no byte outside a request is written.
// No atomics, no workspace, no host synchronisation: one launch each on the caller's stream.
#include <stdio.h>

#include "ws_common.h"
#include "ws_client.h"

#define CL_VERIFY_T 256         // 4 segments per block
#define CL_REQ_T 64
#define CL_ROUND 1024u          // bytes per round: 64 lanes x 16 B

__device__ __forceinline__ u32 cl_byte(uintptr_t a) { return *gptr<unsigned char>(reinterpret_cast<const void*>(a)); }

// ws_cl_field_seq, 64 bytes per step: the delimiter of the field that starts at st (the first
// "\r\n" wholly inside [st, n) when CRLF, else the first ',' in [st, n); none: n) and its trimmed
// bytes [a, b). Wave-uniform arguments and results.
template <bool CRLF>
__device__ __forceinline__ u32 cl_field(uintptr_t base, u32 st, u32 n, u32 lane, u32& a, u32& b) {
    u32 first = WEBSOCKET_CLI_NONE, last = 0, d = n;
    for (u32 r = st; r < n; r += 64) {
        const u32 q = r + lane;
        const u32 c = q < n ? cl_byte(base + q) : 0u;
        bool delim;
        if constexpr (CRLF) {
            u32 nx = (u32)__shfl_down((int)c, 1);
            if (lane == 63) nx = q + 1 < n ? cl_byte(base + q + 1) : 0u;
            delim = q + 1 < n && c == '\r' && nx == '\n';
        } else {
            delim = q < n && c == ',';
        }
        const u64 bd = __ballot(delim);
        u64 bn = __ballot(q < n && !ws_cl_ws(c));
        if (bd) bn &= (1ull << __builtin_ctzll(bd)) - 1ull;           // only the bytes before the delimiter
        if (bn) {
            if (first == WEBSOCKET_CLI_NONE) first = r + (u32)__builtin_ctzll(bn);
            last = r + 63u - (u32)__builtin_clzll(bn);
        }
        if (bd) { d = r + (u32)__builtin_ctzll(bd); break; }
    }
    a = first != WEBSOCKET_CLI_NONE ? first : d;
    b = first != WEBSOCKET_CLI_NONE ? last + 1u : d;
    return d;
}

// ws_cl_list_has_seq for the token "upgrade" in the value [a, b), folded: one element per step
__device__ __forceinline__ bool cl_has_upgrade(uintptr_t base, u32 a, u32 b, u32 lane) {
    for (u32 cur = a;;) {
        u32 x, y;
        const u32 d = cl_field<false>(base, cur, b, lane, x, y);
        if (y - x == 7u) {
            const u32 c = lane < 7u ? ws_cl_fold(cl_byte(base + x + lane)) : 0u;
            if (!__ballot(lane < 7u && c != ws_cl_upgrade_byte(lane))) return true;
        }
        if (d >= b) return false;
        cur = d + 1u;
    }
}

// ws_cl_list_has_seq, case-sensitive, for the value t[0, tlen) in the offered list[0, n)
__device__ __forceinline__ bool cl_offered(uintptr_t list, u32 n, uintptr_t t, u32 tlen, u32 lane) {
    for (u32 cur = 0;;) {
        u32 x, y;
        const u32 d = cl_field<false>(list, cur, n, lane, x, y);
        if (y - x == tlen) {
            u64 diff = 0;
            for (u32 i = 0; i < tlen; i += 64) {
                const u32 k = i + lane;
                diff |= __ballot(k < tlen && cl_byte(list + x + k) != cl_byte(t + k));
            }
            if (!diff) return true;
        }
        if (d >= n) return false;
        cur = d + 1u;
    }
}

// one matched header (its name and ':' at p, inside [0, lim)) into the sweep's state; wave-uniform
__device__ __forceinline__ void cl_header(uintptr_t base, u32 n, int kind, u32 p, const unsigned char* expect, u32 lane,
                                          WsClHeaders& h) {
    const bool first_up = kind == WS_CL_H_UPGRADE && !h.have_up, first_acc = kind == WS_CL_H_ACCEPT && !h.have_acc;
    const bool conn = kind == WS_CL_H_CONNECTION && !h.conn_ok;
    if (!(first_up || first_acc || conn || kind == WS_CL_H_EXTENSIONS || kind == WS_CL_H_PROTOCOL)) return;
    u32 a, b;
    cl_field<true>(base, p + ws_cl_name_len(kind), n, lane, a, b);
    if (first_up) {
        h.have_up = true;
        h.up_ok = false;
        if (b - a == 9u) {
            const u32 c = lane < 9u ? ws_cl_fold(cl_byte(base + a + lane)) : 0u;
            h.up_ok = !__ballot(lane < 9u && c != ws_cl_websocket_byte(lane));
        }
    } else if (conn) {
        h.conn_ok = cl_has_upgrade(base, a, b, lane);
    } else if (first_acc) {
        h.have_acc = true;
        h.acc_off = a;
        h.acc_ok = false;
        if (b - a == WS_HS_ACCEPT_LEN) {
            const bool in = lane < WS_HS_ACCEPT_LEN;
            const u32 c = in ? cl_byte(base + a + lane) : 0u, x = in ? (u32)*gptr<unsigned char>(expect + lane) : 0u;
            h.acc_ok = !__ballot(c != x);
        }
    } else if (kind == WS_CL_H_EXTENSIONS) {
        h.ext_bad = h.ext_bad || b > a;
    } else {
        if (h.nproto++ == 0u) { h.proto_off = a; h.proto_len = b - a; }
    }
}

__device__ __forceinline__ void cl_store_vdesc(WebsocketClientVerifyDesc_t* out, const WebsocketClientVerifyDesc_t& d) {
    u32x4 a, b;
    a.x = (u32)d.ret; a.y = d.reason; a.z = d.status; a.w = d.proto_off;
    b.x = d.proto_len; b.y = d.accept_off; b.z = d.flags; b.w = d.reserved;
    gu32x4* const g = gptr<u32x4>(out);
    g[0] = a;
    g[1] = b;
}

__global__ __launch_bounds__(CL_VERIFY_T) void ws_cl_verify(const unsigned char* buf, u64 buflen, const u64* seg_off,
                                                            const u64* seg_len, u32 nseg, const unsigned char* expect,
                                                            const unsigned char* str, u64 str_len,
                                                            const WebsocketClientEntry_t* entry, u32 max_head,
                                                            WebsocketClientVerifyDesc_t* cv) {
    const u32 lane = threadIdx.x & 63u;
    const u32 s = blockIdx.x * (CL_VERIFY_T / 64) + (threadIdx.x >> 6);
    if (s >= nseg) return;                                           // wave-uniform
    const u64 so = seg_off[s], sl = seg_len[s];
    if (sl >= WS_CL_MAX_SEG || so > buflen || sl > buflen - so) {    // never read
        if (lane == 0) cl_store_vdesc(cv + s, ws_cl_vdesc_rest(-1, WEBSOCKET_CLI_OK, WEBSOCKET_CLI_ERR_SEG_LEN));
        return;
    }
    const u32 n = ws_cl_head_len((u32)sl, max_head);                 // the bytes that may count
    const uintptr_t base = reinterpret_cast<uintptr_t>(buf) + so;
    const u32 lead = (u32)(base & 15u);
    const uintptr_t a0 = base - lead;
    const u64 span = (u64)lead + n;                                  // bytes from a0 to the head's end
    const unsigned char* const exp_s = expect + 32ull * s;
    u32 T = WEBSOCKET_CLI_NONE, L0 = WEBSOCKET_CLI_NONE;
    WsClHeaders h = ws_cl_headers_init();
    for (u64 rb = 0; rb < span && T == WEBSOCKET_CLI_NONE; rb += CL_ROUND) {
        const u64 cb = rb + 16u * lane;                              // this lane's chunk, from a0
        u32x4 v = {0u, 0u, 0u, 0u};
        if (cb < span) v = *gptr<u32x4>(reinterpret_cast<const void*>(a0 + cb));
        u32 nx = (u32)__shfl_down((int)v.x, 1);
        if (lane == 63) nx = cb + 16 < span ? *gptr<u32>(reinterpret_cast<const void*>(a0 + cb + 16)) : 0u;
        const long long lo = (long long)lead - (long long)cb, hi = (long long)span - (long long)cb;
        const WsClChunk c = ws_cl_chunk(v.x, v.y, v.z, v.w, nx, lo, hi);
        const u32 pos = (u32)(cb - lead);                            // (wraps where lo > 0: those bits are masked)
        const u64 bt = __ballot(c.term != 0), bl = __ballot(c.crlf != 0);
        if (bt) T = (u32)__shfl((int)(pos + (c.term ? (u32)__builtin_ctz(c.term) : 0u)), (int)__builtin_ctzll(bt));
        if (bl && L0 == WEBSOCKET_CLI_NONE)
            L0 = (u32)__shfl((int)(pos + (c.crlf ? (u32)__builtin_ctz(c.crlf) : 0u)), (int)__builtin_ctzll(bl));
        const u32 lim = T != WEBSOCKET_CLI_NONE ? T : n;
        // the lanes' candidates against the five names (a handful per response)
        int k0 = 0, k1 = 0;
        u32 p0 = 0, p1 = 0;
        for (u32 m = c.cand; m; m &= m - 1) {
            const u32 p = pos + (u32)__builtin_ctz(m) + 2u;
            if (p + 8u > lim) continue;
            const int kind = ws_cl_name_at(reinterpret_cast<const unsigned char*>(base + p), lim - p);
            if (kind && !k0) { k0 = kind; p0 = p; }
            else if (kind) { k1 = kind; p1 = p; }
        }
        // the round's headers in position order, the whole wave on each
        for (u64 bk = __ballot(k0 != 0); bk; bk &= bk - 1) {
            const int src = (int)__builtin_ctzll(bk);
            cl_header(base, n, __shfl(k0, src), (u32)__shfl((int)p0, src), exp_s, lane, h);
            const int kk = __shfl(k1, src);
            if (kk) cl_header(base, n, kk, (u32)__shfl((int)p1, src), exp_s, lane, h);
        }
    }
    if (T == WEBSOCKET_CLI_NONE) {
        if (lane == 0) cl_store_vdesc(cv + s, ws_cl_vdesc_incomplete(sl, max_head));
        return;
    }
    const u32 mine = lane < 13u && lane < L0 ? cl_byte(base + lane) : 0u;
    u32 f[13], status;
#pragma unroll
    for (int i = 0; i < 13; ++i) f[i] = (u32)__shfl((int)mine, i);
    const bool status_ok = ws_cl_status_line(f, L0, &status);
    bool proto_ok = false;
    if (ws_cl_proto_judged(h) && entry) {
        const gu32x4* const g = gptr<u32x4>(entry + s);
        const u32x4 e0 = g[0], e1 = g[1];
        const u64 off = (u64)e0.z | (u64)e0.w << 32;                 // proto_off
        const u32 plen = e1.w;                                       // proto_len
        if (plen && str && off <= str_len && plen <= str_len - off)
            proto_ok = cl_offered(reinterpret_cast<uintptr_t>(str) + off, plen, base + h.proto_off, h.proto_len, lane);
    }
    if (lane == 0) cl_store_vdesc(cv + s, ws_cl_vdesc(T, status_ok, status, h, proto_ok));
}

// The request's bytes on their way to the slot: 16 at a time in four registers, stored when the
// chunk is full. c counts from the chunk's start; the first chunk begins `lead` bytes into it
// (bytes before the slot are not ours and are not stored).
struct ClFunnel {
    uintptr_t a16;
    u32 c, lead, w0, w1, w2, w3;
    __device__ __forceinline__ void open(unsigned char* dst) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
        a16 = a & ~(uintptr_t)15;
        c = lead = (u32)(a & 15u);
        w0 = w1 = w2 = w3 = 0u;
    }
    __device__ __forceinline__ void store(u32 upto) {
        u32x4 v;
        v.x = w0; v.y = w1; v.z = w2; v.w = w3;
        const u32 cov = ((1u << upto) - 1u) & ~((1u << lead) - 1u);
        if (cov == 0xFFFFu) *gptr<u32x4>(reinterpret_cast<void*>(a16)) = v;
        else if (cov) ws_store_bytes(gptr<unsigned char>(reinterpret_cast<void*>(a16)), v, cov);
    }
    __device__ __forceinline__ void put(u32 b) {
        const u32 d = c >> 2, x = b << (8u * (c & 3u));
        w0 |= d == 0u ? x : 0u;
        w1 |= d == 1u ? x : 0u;
        w2 |= d == 2u ? x : 0u;
        w3 |= d == 3u ? x : 0u;
        if (++c == 16u) {
            store(16u);
            a16 += 16;
            c = lead = 0u;
            w0 = w1 = w2 = w3 = 0u;
        }
    }
    __device__ __forceinline__ void close() { store(c); }
};

__global__ __launch_bounds__(CL_REQ_T) void ws_cl_request(const unsigned char* str, u64 str_len,
                                                          const WebsocketClientEntry_t* entry, const unsigned char* nonce,
                                                          u32 nseg, unsigned char* req, const u64* req_off, u32 req_cap,
                                                          unsigned char* expect, WebsocketClientReqDesc_t* rd) {
    const u32 s = blockIdx.x * CL_REQ_T + threadIdx.x;
    if (s >= nseg) return;
    const gu32x4* const g = gptr<u32x4>(entry + s);
    const u32x4 e0 = g[0], e1 = g[1], e2 = g[2];
    const u64 path_off = (u64)e0.x | (u64)e0.y << 32, proto_off = (u64)e0.z | (u64)e0.w << 32,
              host_off = (u64)e1.x | (u64)e1.y << 32;
    const u32 path_len = e1.z, proto_len = e1.w, host_len = e2.x;
    const bool in = (!path_len || (path_off <= str_len && path_len <= str_len - path_off)) &&
                    (!proto_len || (proto_off <= str_len && proto_len <= str_len - proto_off)) &&
                    (!host_len || (host_off <= str_len && host_len <= str_len - host_off));
    const unsigned char *const path = str + path_off, *const proto = str + proto_off, *const host = str + host_off;
    u32 err = in ? 0u : WEBSOCKET_CLI_ERR_RANGE;
    if (in) err = ws_cl_check_bytes(path, path_len, proto, proto_len, host, host_len);
    const WebsocketClientReqDesc_t d = ws_cl_req_desc(err, path_len, proto_len, host_len, req != nullptr, req_cap);
    u32x4 dv;
    dv.x = d.req_len; dv.y = d.key_off; dv.z = d.flags; dv.w = d.reserved;
    *gptr<u32x4>(rd + s) = dv;
    if (d.flags & (WEBSOCKET_CLI_ERR_RANGE | WEBSOCKET_CLI_ERR_BYTES)) return;
    const u32x4 nv = *gptr<u32x4>(nonce + 16ull * s);
    const u32 nw[4] = {nv.x, nv.y, nv.z, nv.w};
    u32 key[6], acc[8];
    ws_cl_key(nw, key);
    ws_cl_expect(key, acc);
    gu32x4* const ga = gptr<u32x4>(expect + 32ull * s);
    u32x4 lo4, hi4;
    lo4.x = acc[0]; lo4.y = acc[1]; lo4.z = acc[2]; lo4.w = acc[3];
    hi4.x = acc[4]; hi4.y = acc[5]; hi4.z = acc[6]; hi4.w = 0u;
    ga[0] = lo4;
    ga[1] = hi4;
    if (!(d.flags & WEBSOCKET_CLI_REQ_WRITTEN)) return;
    ClFunnel o;
    o.open(req + (req_off ? req_off[s] : (u64)s * req_cap));
    ws_cl_emit_request(o, path, path_len, proto, proto_len, host, host_len, key);
    o.close();
}

static int cl_flags(const char* who, unsigned int flags) {
    static thread_local char msg[128];
    if (!flags) return 0;
    snprintf(msg, sizeof(msg), "%s: unknown flag", who);
    return ws_set_msg(msg);
}

extern "C" WSFRAME_AMD_CLI_EXPORT int websocketframeBatchClientRequestDevice(
    const unsigned char* d_str, unsigned long long str_len, const WebsocketClientEntry_t* d_entry,
    const unsigned char* d_nonce, unsigned int nseg, unsigned int flags, unsigned char* d_req,
    const unsigned long long* d_req_off, unsigned int req_cap, unsigned char* d_expect, WebsocketClientReqDesc_t* d_rd,
    void* hip_stream) {
    if (cl_flags("websocketframeBatchClientRequestDevice", flags)) return -1;
    if (nseg == 0) return 0;
    if (!d_entry || !d_nonce || !d_expect || !d_rd || (!d_str && str_len))
        return ws_set_msg("websocketframeBatchClientRequestDevice: invalid argument");
    if ((reinterpret_cast<uintptr_t>(d_entry) | reinterpret_cast<uintptr_t>(d_nonce) | reinterpret_cast<uintptr_t>(d_expect) |
         reinterpret_cast<uintptr_t>(d_rd)) & 15)
        return ws_set_msg("websocketframeBatchClientRequestDevice: d_entry/d_nonce/d_expect/d_rd not 16-B aligned");
    if (reinterpret_cast<uintptr_t>(d_req_off) & 7)
        return ws_set_msg("websocketframeBatchClientRequestDevice: d_req_off not 8-B aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(ws_cl_request, dim3((nseg + CL_REQ_T - 1) / CL_REQ_T), dim3(CL_REQ_T), 0, st, d_str, (u64)str_len,
                       d_entry, d_nonce, nseg, d_req, d_req_off, req_cap, d_expect, d_rd);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchClientRequestDevice launch", e);
}

extern "C" WSFRAME_AMD_CLI_EXPORT int websocketframeBatchClientVerifyDevice(
    const unsigned char* d_buf, unsigned long long buflen, const unsigned long long* d_seg_off,
    const unsigned long long* d_seg_len, unsigned int nseg, unsigned int flags, const unsigned char* d_expect,
    const unsigned char* d_str, unsigned long long str_len, const WebsocketClientEntry_t* d_entry, unsigned int max_head,
    WebsocketClientVerifyDesc_t* d_cv, void* hip_stream) {
    if (cl_flags("websocketframeBatchClientVerifyDevice", flags)) return -1;
    if (nseg == 0) return 0;
    if (!d_buf || !d_seg_off || !d_seg_len || !d_expect || !d_cv)
        return ws_set_msg("websocketframeBatchClientVerifyDevice: invalid argument");
    if ((reinterpret_cast<uintptr_t>(d_cv) | reinterpret_cast<uintptr_t>(d_expect) | reinterpret_cast<uintptr_t>(d_entry)) & 15)
        return ws_set_msg("websocketframeBatchClientVerifyDevice: d_cv/d_expect/d_entry not 16-B aligned");
    if ((reinterpret_cast<uintptr_t>(d_seg_off) | reinterpret_cast<uintptr_t>(d_seg_len)) & 7)
        return ws_set_msg("websocketframeBatchClientVerifyDevice: d_seg_off/d_seg_len not 8-B aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(ws_cl_verify, dim3((nseg + CL_VERIFY_T / 64 - 1) / (CL_VERIFY_T / 64)), dim3(CL_VERIFY_T), 0, st, d_buf,
                       (u64)buflen, d_seg_off, d_seg_len, nseg, d_expect, d_str, (u64)str_len, d_entry, max_head, d_cv);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchClientVerifyDevice launch", e);
}

extern "C" WSFRAME_AMD_CLI_EXPORT int websocketframeClientRequestHost(
    const unsigned char* path, unsigned int path_len, const unsigned char* proto, unsigned int proto_len,
    const unsigned char* host, unsigned int host_len, const unsigned char nonce[16], unsigned int flags,
    unsigned char* req, unsigned int req_cap, unsigned char expect[32], WebsocketClientReqDesc_t* rd) {
    if (cl_flags("websocketframeClientRequestHost", flags)) return -1;
    if (!rd || !expect || !nonce || (!path && path_len) || (!proto && proto_len) || (!host && host_len))
        return ws_set_msg("websocketframeClientRequestHost: invalid argument");
    ws_cl_request_one(path, path_len, proto, proto_len, host, host_len, nonce, req, req_cap, expect, rd);
    return 0;
}

extern "C" WSFRAME_AMD_CLI_EXPORT int websocketframeClientVerifyHost(
    const unsigned char* buf, unsigned int len, unsigned int flags, const unsigned char expect[32],
    const unsigned char* offered, unsigned int offered_len, unsigned int max_head, WebsocketClientVerifyDesc_t* cv) {
    if (cl_flags("websocketframeClientVerifyHost", flags)) return -1;
    if (!cv || !expect || (!buf && len)) return ws_set_msg("websocketframeClientVerifyHost: invalid argument");
    ws_cl_verify_one(buf, len, expect, offered, offered_len, max_head, cv);
    return 0;
}
