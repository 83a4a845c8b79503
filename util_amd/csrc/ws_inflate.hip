// ws_inflate.hip — websocketframeBatchInflateDevice, websocketframeBatchInflateListFromMessagesDevice
// and websocketframeInflateHost (include/wsframe_amd_deflate.h): permessage-deflate bodies inflated
// per connection, for gfx950. The rule — the DEFLATE decoder, zlib's verdicts, the limits, the walk
// over a connection's list — is ws_inflate.h's (one definition, host-tested); this file is its Io
// for one wavefront.
//
// DEFLATE is serial inside a stream; the parallelism is over connections. A fixed grid of
// wavefronts (4 per workgroup) takes connections by index, one wave walks its connection's entries
// in order. Every value of the decoder is wave-uniform (uni() is readfirstlane, so the symbol loop
// branches on scalars):
//   tables   per wave in LDS (2.2 KiB: the block's lookups, counts and symbols, the header scratch);
//            lane 0 stores the words of the serial construction, the 64 lanes share the lookup
//            fill. The fixed code is built once per workgroup.
//   input    a 256-byte window of the body in LDS, refilled by one 64-lane load of aligned dwords
//            (the dwords that straddle the body's ends byte by byte, inside the body only);
//   output   literals gather in a 64-byte LDS run and leave as one store per run; a match is a
//            wave-wide copy, lane k writing out[pos + k] = out[pos - dist + k % dist], which reads
//            only bytes before pos (so dist < len needs no serial loop); a stored block is 16-B
//            chunks from the destination's first aligned byte on;
//   history  is the message's own output in d_dst. A match's source was stored by other lanes of
//            the same wave: before such a load the wave waits for its stores (vmcnt(0)) and
//            fences at workgroup scope — the CU's L1 is shared by the wave's lanes, so no
//            invalidate is needed. The wait is skipped while the source lies wholly below the
//            position the last wait covered.
// Every output is written with plain vector stores; the call needs no workspace.
#include <stdio.h>

#include "ws_common.h"
#include "ws_inflate.h"

#define INF_WAVES 4                      // wavefronts (connections in flight) per workgroup
#define INF_T (64 * INF_WAVES)
#define INF_BLOCKS_PER_CU 8              // the fixed grid
#define INF_WIN 256u                     // input window bytes

static_assert(sizeof(WebsocketInflateMsg_t) == 24 && sizeof(WebsocketInflateMsgRes_t) == 24 &&
                  sizeof(WebsocketInflateResult_t) == 24 && sizeof(WsInfTabs) == 1856,
              "record sizes");

typedef u32x4 __attribute__((aligned(1))) inf_u32x4u;

struct InfLds {                          // one wave's
    WsInfTabs T;
    WsInfWork W;
    u32 win[INF_WIN / 4];
    unsigned char lit[64];
};

// stores of this wave complete before its later loads (see the head comment)
__device__ __forceinline__ void inf_fence() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

struct InfIo {
    u32 ln;
    const unsigned char* src;            // the message's body
    u64 len;
    unsigned char* dst;                  // the message's first output byte
    u32* win;
    unsigned char* litb;
    long long wb;                        // the window holds body bytes [wb, wb + INF_WIN)
    u32 nlit;
    u64 litpos, fenced;                  // the run's first position; stores below `fenced` are complete

    __device__ __forceinline__ u32 uni(u32 v) const { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ u32 lane() const { return ln; }
    __device__ __forceinline__ u32 lanes() const { return 64; }
    __device__ __forceinline__ void sync() {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void st16(wsinf_u16* p, wsinf_u16 v) { if (ln == 0) *p = v; }
    __device__ __forceinline__ void st8(wsinf_u8* p, wsinf_u8 v) { if (ln == 0) *p = v; }
    __device__ __forceinline__ void put16(wsinf_u16* p, wsinf_u16 v) { *p = v; }
    __device__ __forceinline__ void put8(wsinf_u8* p, wsinf_u8 v) { *p = v; }

    __device__ __forceinline__ void load_window(u64 i) {
        const u32 a = (u32)(reinterpret_cast<uintptr_t>(src + i) & 3u);
        wb = (long long)i - (long long)a;
        const long long off = wb + 4ll * ln;
        u32 v = 0;
        if (off >= 0 && (u64)off + 4 <= len) {
            v = *gptr<u32>(src + off);
        } else {
            for (u32 j = 0; j < 4; ++j)
                if (off + j >= 0 && (u64)(off + j) < len) v |= (u32)*gptr<unsigned char>(src + off + j) << (8u * j);
        }
        sync();
        win[ln] = v;
        sync();
    }
    __device__ __forceinline__ u32 in_byte(u64 i) {
        long long r = (long long)i - wb;
        if (r < 0 || r >= (long long)INF_WIN) {
            load_window(i);
            r = (long long)i - wb;
        }
        return uni((win[(u32)r >> 2] >> (8u * ((u32)r & 3u))) & 0xFFu);
    }

    __device__ __forceinline__ void flush() {
        if (nlit) {
            sync();
            if (ln < nlit) *gptr<unsigned char>(dst + litpos + ln) = litb[ln];
            nlit = 0;
            sync();
        }
    }
    __device__ __forceinline__ void lit(u64 pos, u32 v) {
        if (nlit == 0) litpos = pos;
        if (ln == 0) litb[nlit] = (unsigned char)v;
        if (++nlit == 64) flush();
    }
    __device__ __forceinline__ void match(u64 pos, u32 dist, u32 n) {
        flush();
        if (pos - dist + (n < dist ? n : dist) > fenced) {
            inf_fence();
            fenced = pos;
        }
        const unsigned char* const from = dst + pos - dist;
        for (u32 k = ln; k < n; k += 64) {
            const u32 j = dist < n ? k % dist : k;
            *gptr<unsigned char>(dst + pos + k) = *gptr<unsigned char>(from + j);
        }
    }
    __device__ __forceinline__ void stored(u64 pos, u64 at, u32 n) {
        flush();
        unsigned char* const to = dst + pos;
        const unsigned char* const from = src + at;
        u32 head = (u32)(-reinterpret_cast<uintptr_t>(to)) & 15u;
        if (head > n) head = n;
        const u32 nq = (n - head) >> 4, tail0 = head + (nq << 4);
        if (ln < head) *gptr<unsigned char>(to + ln) = *gptr<unsigned char>(from + ln);
        for (u32 q = ln; q < nq; q += 64)
            *gptr<u32x4>(to + head + 16u * q) =
                *reinterpret_cast<const WS_GLOBAL inf_u32x4u*>(reinterpret_cast<uintptr_t>(from + head + 16u * q));
        if (tail0 + ln < n) *gptr<unsigned char>(to + tail0 + ln) = *gptr<unsigned char>(from + tail0 + ln);
    }
};

struct InfConn {
    u32 ln;
    const unsigned char* src;
    const WebsocketInflateMsg_t* msg;    // the connection's first entry
    unsigned char* dst;
    WebsocketInflateMsgRes_t* res;
    u64 limit;
    InfLds* L;
    const WsInfTabs* F;

    __device__ __forceinline__ WebsocketInflateMsg_t entry(u32 i) const {
        const gu64* const g = gptr<u64>(msg + i);
        WebsocketInflateMsg_t m;
        m.src_off = g[0];
        m.len = g[1];
        m.kind = (u32)g[2];
        m.reserved = 0;
        return m;
    }
    __device__ __forceinline__ void result(u32 i, const WebsocketInflateMsgRes_t& r) {
        if (ln == 0) {
            gu64* const g = gptr<u64>(res + i);
            g[0] = r.out_off;
            g[1] = r.out_len;
            g[2] = (u64)r.status;
        }
    }
    __device__ __forceinline__ u32 inflate(const WebsocketInflateMsg_t& m, u64 out_off, u64 room, u64* got) {
        InfIo io;
        io.ln = ln;
        io.src = src + m.src_off;
        io.len = m.len;
        io.dst = dst + out_off;
        io.win = L->win;
        io.litb = L->lit;
        io.wb = -(long long)(2 * INF_WIN);
        io.nlit = 0;
        io.litpos = 0;
        io.fenced = 0;
        const u32 st = ws_inflate_message(io, m.len, limit, room, &L->T, F, &L->W, got);
        io.flush();
        return st;
    }
};

__global__ __launch_bounds__(INF_T) void ws_inflate_kernel(const unsigned char* src, u64 src_len, const WebsocketInflateMsg_t* msg,
                                                           const u32* nmsg, u32 nseg, u32 max_msgs, u64 limit, unsigned char* dst,
                                                           const u64* dst_off, const u64* dst_cap, WebsocketInflateMsgRes_t* msg_res,
                                                           WebsocketInflateResult_t* res) {
    __shared__ InfLds lds[INF_WAVES];
    __shared__ WsInfTabs fixed;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    if (wave == 0) {
        InfIo io;
        io.ln = lane;
        ws_inf_build_fixed(io, &fixed, &lds[0].W);
    }
    __syncthreads();
    for (u64 s64 = (u64)blockIdx.x * INF_WAVES + wave; s64 < nseg; s64 += (u64)gridDim.x * INF_WAVES) {
        const u32 s = (u32)s64;
        const u32 cnt = *gptr<u32>(nmsg + s), n = cnt < max_msgs ? cnt : max_msgs;
        InfConn c;
        c.ln = lane;
        c.src = src;
        c.msg = msg + (u64)s * max_msgs;
        c.dst = dst;
        c.res = msg_res + (u64)s * max_msgs;
        c.limit = limit;
        c.L = &lds[wave];
        c.F = &fixed;
        const WebsocketInflateResult_t R = ws_inflate_walk(c, n, src_len, *gptr<u64>(dst_off + s), *gptr<u64>(dst_cap + s));
        if (lane == 0) {
            gu64* const g = gptr<u64>(res + s);
            g[0] = R.out_len;
            g[1] = (u64)R.n_msgs | (u64)R.status << 32;
            g[2] = (u64)R.first_bad | (u64)R.close_status << 32;
        }
    }
}

// the inflate list from reassembly's messages: slot (s, i) from message i of connection s
__global__ __launch_bounds__(INF_T) void ws_inflate_list(const unsigned char* buf, const WebsocketFrameDesc_t* desc,
                                                         const WebsocketMsgDesc_t* msg, const u32* nmsg, u32 nslots, u32 max_frames,
                                                         WebsocketInflateMsg_t* out) {
    const u64 q64 = (u64)blockIdx.x * INF_T + threadIdx.x;
    if (q64 >= nslots) return;
    const u32 q = (u32)q64, s = q / max_frames, i = q - s * max_frames;
    const u32 cnt = *gptr<u32>(nmsg + s);
    u64 off = 0, len = 0;
    u32 kind = WEBSOCKET_INFLATE_SKIP;
    if (i < (cnt < max_frames ? cnt : max_frames)) {
        const gu32x4* const g = gptr<u32x4>(msg + q);
        const u32x4 a = g[0], b = g[1];                    // out_off, len | first_frame, n_frames, complete, continued
        if (b.z && !b.w && b.x < max_frames) {
            const gu32x4* const d = gptr<u32x4>(desc + ((u64)s * max_frames + b.x));
            const u32x4 d0 = d[0];                         // frame_off, data_off
            const u32 t = (d[1].w >> 8) & 0xFFu;
            if ((t == 1u || t == 2u) && (*gptr<unsigned char>(buf + ((u64)d0.x | (u64)d0.y << 32)) & 0x40u)) {
                kind = WEBSOCKET_INFLATE_RAW;
                off = (u64)a.x | (u64)a.y << 32;
                len = (u64)a.z | (u64)a.w << 32;
            }
        }
    }
    gu64* const o = gptr<u64>(out + q);
    o[0] = off;
    o[1] = len;
    o[2] = (u64)kind;
}

extern "C" WSFRAME_AMD_DEFLATE_EXPORT int websocketframeBatchInflateDevice(
    const unsigned char* d_src, unsigned long long src_len, const WebsocketInflateMsg_t* d_msg, const unsigned int* d_nmsg,
    unsigned int nseg, unsigned int max_msgs, unsigned long long max_message_size, unsigned int flags, unsigned char* d_dst,
    const unsigned long long* d_dst_off, const unsigned long long* d_dst_cap, WebsocketInflateMsgRes_t* d_msg_res,
    WebsocketInflateResult_t* d_res, void* hip_stream) {
    if (flags) return ws_set_msg("websocketframeBatchInflateDevice: unknown flag");
    if (max_msgs == 0) return ws_set_msg("websocketframeBatchInflateDevice: invalid argument (max_msgs 0)");
    if (nseg == 0) return 0;
    if (!d_src || !d_msg || !d_nmsg || !d_dst || !d_dst_off || !d_dst_cap || !d_msg_res || !d_res)
        return ws_set_msg("websocketframeBatchInflateDevice: invalid argument (NULL pointer)");
    if ((reinterpret_cast<uintptr_t>(d_msg) | reinterpret_cast<uintptr_t>(d_dst_off) | reinterpret_cast<uintptr_t>(d_dst_cap) |
         reinterpret_cast<uintptr_t>(d_msg_res) | reinterpret_cast<uintptr_t>(d_res)) & 7)
        return ws_set_msg("websocketframeBatchInflateDevice: d_msg/d_dst_off/d_dst_cap/d_msg_res/d_res not 8-B aligned");
    if (reinterpret_cast<uintptr_t>(d_nmsg) & 3) return ws_set_msg("websocketframeBatchInflateDevice: d_nmsg not 4-B aligned");
    if ((u64)nseg * max_msgs > (1ull << 30)) return ws_set_msg("websocketframeBatchInflateDevice: nseg * max_msgs > 2^30");
    int cus = 0, lds = 0;
    const int rc = ws_device_info(&cus, &lds);
    if (rc) return rc;
    const u32 want = (nseg + INF_WAVES - 1) / INF_WAVES, gcap = (u32)cus * INF_BLOCKS_PER_CU, grid = want < gcap ? want : gcap;
    hipLaunchKernelGGL(ws_inflate_kernel, dim3(grid), dim3(INF_T), 0, reinterpret_cast<hipStream_t>(hip_stream), d_src, (u64)src_len,
                       d_msg, d_nmsg, nseg, max_msgs, (u64)max_message_size, d_dst, reinterpret_cast<const u64*>(d_dst_off),
                       reinterpret_cast<const u64*>(d_dst_cap), d_msg_res, d_res);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchInflateDevice launch", e);
}

extern "C" WSFRAME_AMD_DEFLATE_EXPORT int websocketframeBatchInflateListFromMessagesDevice(
    const unsigned char* d_buf, const WebsocketFrameDesc_t* d_desc, const WebsocketMsgDesc_t* d_msg, const unsigned int* d_nmsg,
    unsigned int nseg, unsigned int max_frames, WebsocketInflateMsg_t* d_inf_msg, void* hip_stream) {
    if (max_frames == 0) return ws_set_msg("websocketframeBatchInflateListFromMessagesDevice: invalid argument (max_frames 0)");
    if (!d_buf || !d_desc || !d_msg || !d_nmsg || !d_inf_msg)
        return ws_set_msg("websocketframeBatchInflateListFromMessagesDevice: invalid argument (NULL pointer)");
    if ((reinterpret_cast<uintptr_t>(d_desc) | reinterpret_cast<uintptr_t>(d_msg)) & 15)
        return ws_set_msg("websocketframeBatchInflateListFromMessagesDevice: d_desc/d_msg not 16-B aligned");
    if ((reinterpret_cast<uintptr_t>(d_inf_msg) & 7) || (reinterpret_cast<uintptr_t>(d_nmsg) & 3))
        return ws_set_msg("websocketframeBatchInflateListFromMessagesDevice: d_inf_msg not 8-B or d_nmsg not 4-B aligned");
    const u64 nslots = (u64)nseg * max_frames;
    if (nslots > (1ull << 30)) return ws_set_msg("websocketframeBatchInflateListFromMessagesDevice: nseg * max_frames > 2^30");
    if (nslots == 0) return 0;
    hipLaunchKernelGGL(ws_inflate_list, dim3((u32)((nslots + INF_T - 1) / INF_T)), dim3(INF_T), 0,
                       reinterpret_cast<hipStream_t>(hip_stream), d_buf, d_desc, d_msg, d_nmsg, (u32)nslots, max_frames, d_inf_msg);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchInflateListFromMessagesDevice launch", e);
}

extern "C" WSFRAME_AMD_DEFLATE_EXPORT long long websocketframeInflateHost(
    const unsigned char* src, unsigned long long src_len, const WebsocketInflateMsg_t* msg, unsigned int nmsg,
    unsigned long long max_message_size, unsigned int flags, unsigned char* dst, unsigned long long dst_cap,
    WebsocketInflateMsgRes_t* msg_res, WebsocketInflateResult_t* out) {
    if (flags) return ws_set_msg("websocketframeInflateHost: unknown flag");
    if (!out || (!src && src_len) || (!msg && nmsg) || (!dst && dst_cap))
        return ws_set_msg("websocketframeInflateHost: invalid argument (NULL pointer)");
    return (long long)ws_inflate_connection(src, src_len, msg, nmsg, max_message_size, dst, dst_cap, msg_res, out);
}
