// ws_deflate.hip — websocketframeBatchDeflateDevice, websocketframeBatchSendListFromDeflatedDevice
// and websocketframeDeflateHost (include/wsframe_amd_compress.h): the messages of a send list
// compressed as permessage-deflate bodies, every message into a room of its own, for gfx950. The
// rule — hash, lookup before insert, highest position wins, greedy choice, fixed Huffman codes, the
// verdict, which bytes of the room are written — is ws_deflate.h's (one definition, host-tested);
// this file is its Io for one wavefront.
//
// With no context takeover every message is a stream of its own: the parallelism is over
// messages, and inside a message over the 64 positions of a group. A fixed grid of wavefronts
// (4 per workgroup) takes the message slots s * max_msgs + i by index; one wave compresses one
// message, a position per lane:
//   input    every lane loads the 4 bytes at its position straight from d_src (an unaligned dword
//            load; the 64 loads of a group share two or three cache lines), the match compare
//            walks on 4 bytes at a time, inside the message's range only;
//   table    per wave in LDS (8 KiB of positions; a message shorter than 2 KiB clears and uses a
//            part of it). A group's inserts are a plain store and an LDS max, so the highest
//            position holds the slot whichever lane's store landed last;
//   choose   ballot of the lanes that hold a match, then a scalar loop over the chosen matches
//            (count trailing zeros, readlane of the match length): at most 16 turns per group;
//   pack     token bit lengths prefix-summed across the wave (6 shuffle steps), every lane ORs its
//            token into one or two words of a 264-byte LDS staging buffer (LDS or), whole words
//            leave as aligned dword stores, the room's unaligned ends byte by byte;
//   PLAIN    a message that does not shrink is copied again from d_src, which never overlaps the
//            rooms: 16-B chunks from the room's first aligned byte on.
// Every output is written with plain vector stores; the call needs no workspace. The LDS table and
// staging words of a wave are read after other lanes' stores only behind sync() (a wavefront-scope
// fence: the wave's LDS operations complete in order).
#include <stdio.h>

#include "ws_common.h"
#include "ws_deflate.h"

#define DEF_WAVES 4                      // wavefronts (messages in flight) per workgroup
#define DEF_T (64 * DEF_WAVES)
#define DEF_BLOCKS_PER_CU 4              // the fixed grid: 16 waves per CU, 33 KiB of LDS per workgroup

static_assert(sizeof(WebsocketDeflateMsg_t) == 24 && sizeof(WebsocketDeflateMsgRes_t) == 24 && sizeof(WsDefWork) == 8456, "record sizes");
static_assert(WS_DEF_GROUP == 64, "a group is a wavefront");

typedef u32x4 __attribute__((aligned(1))) def_u32x4u;
typedef u32 __attribute__((aligned(1))) def_u32u;

__device__ __forceinline__ u64 def_uni64(u64 v) {
    return (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)v) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32)) << 32;
}

struct DefIo {
    static const u32 NL = 1;
    u32 ln;
    const unsigned char* src;            // the message's body
    unsigned char* dst;                  // the room's first byte

    __device__ __forceinline__ u32 l0() const { return ln; }
    __device__ __forceinline__ u32 l1() const { return ln + 1; }
    __device__ __forceinline__ u32 lane() const { return ln; }
    __device__ __forceinline__ u32 lanes() const { return 64; }
    __device__ __forceinline__ u32 uni(u32 v) const { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ void sync() {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ u32 phase() const { return uni((u32)(reinterpret_cast<uintptr_t>(dst) & 3u)); }
    __device__ __forceinline__ u32 ld8(u64 i) const { return *gptr<unsigned char>(src + i); }
    __device__ __forceinline__ u32 ld32(u64 i) const {
        return *reinterpret_cast<const WS_GLOBAL def_u32u*>(reinterpret_cast<uintptr_t>(src + i));
    }
    __device__ __forceinline__ void put32(u32* p, u32 v) { *p = v; }
    __device__ __forceinline__ void max32(u32* p, u32 v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
    __device__ __forceinline__ void or32(u32* p, u32 v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
    __device__ __forceinline__ u64 ballot(const bool* f) const { return __ballot(f[0]); }
    __device__ __forceinline__ u32 bcast(const u32* v, u32 j) const { return (u32)__builtin_amdgcn_readlane((int)v[0], (int)j); }
    __device__ __forceinline__ u32 scan(const u32* v, u32* excl) const {
        u32 s = v[0];
        for (u32 d = 1; d < 64; d <<= 1) {
            const u32 t = (u32)__shfl_up((int)s, d, 64);
            if (ln >= d) s += t;
        }
        excl[0] = s - v[0];
        return (u32)__builtin_amdgcn_readlane((int)s, 63);
    }
    __device__ __forceinline__ void out_word(u64 q, u32 v) { *gptr<u32>(dst + q) = v; }
    __device__ __forceinline__ void out_byte(u64 q, u32 v) { *gptr<unsigned char>(dst + q) = (unsigned char)v; }
    __device__ __forceinline__ void copy(u64 n) {
        u64 head = (u64)(-reinterpret_cast<uintptr_t>(dst)) & 15u;
        if (head > n) head = n;
        const u64 nq = (n - head) >> 4, tail0 = head + (nq << 4);
        if (ln < head) *gptr<unsigned char>(dst + ln) = *gptr<unsigned char>(src + ln);
        for (u64 q = ln; q < nq; q += 64)
            *gptr<u32x4>(dst + head + 16u * q) =
                *reinterpret_cast<const WS_GLOBAL def_u32x4u*>(reinterpret_cast<uintptr_t>(src + head + 16u * q));
        if (tail0 + ln < n) *gptr<unsigned char>(dst + tail0 + ln) = *gptr<unsigned char>(src + tail0 + ln);
    }
};

struct DefSlot {
    u32 ln;
    const unsigned char* src;
    unsigned char* dst;
    WsDefWork* W;
    __device__ __forceinline__ u32 deflate(const WebsocketDeflateMsg_t& m, u64 off, u64 cap, u64 min_len, u64* out_len) {
        DefIo io;
        io.ln = ln;
        io.src = src + m.src_off;
        io.dst = dst + off;
        u64 enc = 0;
        return ws_deflate_message(io, m.len, cap, min_len, W, out_len, &enc);
    }
};

__global__ __launch_bounds__(DEF_T) void ws_deflate_kernel(const unsigned char* src, u64 src_len, const WebsocketDeflateMsg_t* msg,
                                                           const u32* nmsg, u32 nslots, u32 max_msgs, u64 min_len, unsigned char* dst,
                                                           const u64* dst_off, const u64* dst_cap, WebsocketDeflateMsgRes_t* msg_res) {
    __shared__ WsDefWork lds[DEF_WAVES];
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    for (u64 q64 = (u64)blockIdx.x * DEF_WAVES + wave; q64 < nslots; q64 += (u64)gridDim.x * DEF_WAVES) {
        const u32 q = (u32)q64, s = q / max_msgs, i = q - s * max_msgs;
        const u32 cnt = (u32)__builtin_amdgcn_readfirstlane((int)*gptr<u32>(nmsg + s));
        if (i >= (cnt < max_msgs ? cnt : max_msgs)) continue;
        const gu64* const g = gptr<u64>(msg + q);
        WebsocketDeflateMsg_t m;                               // (every lane loads the same words: scalars for the rule's loops)
        m.src_off = def_uni64(g[0]);
        m.len = def_uni64(g[1]);
        m.type = (u32)def_uni64(g[2]);
        m.reserved = 0;
        DefSlot c;
        c.ln = lane;
        c.src = src;
        c.dst = dst;
        c.W = &lds[wave];
        const WebsocketDeflateMsgRes_t r =
            ws_deflate_entry(c, m, src_len, min_len, def_uni64(*gptr<u64>(dst_off + q)), def_uni64(*gptr<u64>(dst_cap + q)));
        if (lane == 0) {
            gu64* const o = gptr<u64>(msg_res + q);
            o[0] = r.out_off;
            o[1] = r.out_len;
            o[2] = (u64)r.status;
        }
    }
}

// the send list of the compressed messages: slot (s, i) from its entry and its result
__global__ __launch_bounds__(DEF_T) void ws_deflate_send_list(const WebsocketDeflateMsg_t* msg, const u32* nmsg, u32 nslots, u32 max_msgs,
                                                              const WebsocketDeflateMsgRes_t* msg_res, WebsocketSendMsg_t* out) {
    const u64 q64 = (u64)blockIdx.x * DEF_T + threadIdx.x;
    if (q64 >= nslots) return;
    const u32 q = (u32)q64, s = q / max_msgs, i = q - s * max_msgs;
    const u32 cnt = *gptr<u32>(nmsg + s);
    if (i >= (cnt < max_msgs ? cnt : max_msgs)) return;
    const gu64* const g = gptr<u64>(msg_res + q);
    WebsocketDeflateMsgRes_t r;
    r.out_off = g[0];
    r.out_len = g[1];
    r.status = (u32)g[2];
    r.reserved = 0;
    const WebsocketSendMsg_t e = ws_deflate_send_entry((u32)gptr<u64>(msg + q)[2], r);
    gu64* const o = gptr<u64>(out + q);
    o[0] = e.src_off;
    o[1] = e.len;
    o[2] = (u64)e.type;
}

extern "C" WSFRAME_AMD_PMD_EXPORT int websocketframeBatchDeflateDevice(
    const unsigned char* d_src, unsigned long long src_len, const WebsocketDeflateMsg_t* d_msg, const unsigned int* d_nmsg,
    unsigned int nseg, unsigned int max_msgs, unsigned long long min_len, unsigned int flags, unsigned char* d_dst,
    const unsigned long long* d_dst_off, const unsigned long long* d_dst_cap, WebsocketDeflateMsgRes_t* d_msg_res, void* hip_stream) {
    if (flags) return ws_set_msg("websocketframeBatchDeflateDevice: unknown flag");
    if (max_msgs == 0) return ws_set_msg("websocketframeBatchDeflateDevice: invalid argument (max_msgs 0)");
    if (nseg == 0) return 0;
    if (!d_src || !d_msg || !d_nmsg || !d_dst || !d_dst_off || !d_dst_cap || !d_msg_res)
        return ws_set_msg("websocketframeBatchDeflateDevice: invalid argument (NULL pointer)");
    if ((reinterpret_cast<uintptr_t>(d_msg) | reinterpret_cast<uintptr_t>(d_dst_off) | reinterpret_cast<uintptr_t>(d_dst_cap) |
         reinterpret_cast<uintptr_t>(d_msg_res)) & 7)
        return ws_set_msg("websocketframeBatchDeflateDevice: d_msg/d_dst_off/d_dst_cap/d_msg_res not 8-B aligned");
    if (reinterpret_cast<uintptr_t>(d_nmsg) & 3) return ws_set_msg("websocketframeBatchDeflateDevice: d_nmsg not 4-B aligned");
    const u64 nslots = (u64)nseg * max_msgs;
    if (nslots > (1ull << 30)) return ws_set_msg("websocketframeBatchDeflateDevice: nseg * max_msgs > 2^30");
    int cus = 0, lds = 0;
    const int rc = ws_device_info(&cus, &lds);
    if (rc) return rc;
    const u32 want = (u32)((nslots + DEF_WAVES - 1) / DEF_WAVES), gcap = (u32)cus * DEF_BLOCKS_PER_CU, grid = want < gcap ? want : gcap;
    hipLaunchKernelGGL(ws_deflate_kernel, dim3(grid), dim3(DEF_T), 0, reinterpret_cast<hipStream_t>(hip_stream), d_src, (u64)src_len,
                       d_msg, d_nmsg, (u32)nslots, max_msgs, (u64)min_len, d_dst, reinterpret_cast<const u64*>(d_dst_off),
                       reinterpret_cast<const u64*>(d_dst_cap), d_msg_res);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchDeflateDevice launch", e);
}

extern "C" WSFRAME_AMD_PMD_EXPORT int websocketframeBatchSendListFromDeflatedDevice(
    const WebsocketDeflateMsg_t* d_msg, const unsigned int* d_nmsg, unsigned int nseg, unsigned int max_msgs,
    const WebsocketDeflateMsgRes_t* d_msg_res, WebsocketSendMsg_t* d_send_msg, void* hip_stream) {
    if (max_msgs == 0) return ws_set_msg("websocketframeBatchSendListFromDeflatedDevice: invalid argument (max_msgs 0)");
    if (nseg && (!d_msg || !d_nmsg || !d_msg_res || !d_send_msg))
        return ws_set_msg("websocketframeBatchSendListFromDeflatedDevice: invalid argument (NULL pointer)");
    if ((reinterpret_cast<uintptr_t>(d_msg) | reinterpret_cast<uintptr_t>(d_msg_res) | reinterpret_cast<uintptr_t>(d_send_msg)) & 7)
        return ws_set_msg("websocketframeBatchSendListFromDeflatedDevice: d_msg/d_msg_res/d_send_msg not 8-B aligned");
    if (reinterpret_cast<uintptr_t>(d_nmsg) & 3) return ws_set_msg("websocketframeBatchSendListFromDeflatedDevice: d_nmsg not 4-B aligned");
    const u64 nslots = (u64)nseg * max_msgs;
    if (nslots > (1ull << 30)) return ws_set_msg("websocketframeBatchSendListFromDeflatedDevice: nseg * max_msgs > 2^30");
    if (nslots == 0) return 0;
    hipLaunchKernelGGL(ws_deflate_send_list, dim3((u32)((nslots + DEF_T - 1) / DEF_T)), dim3(DEF_T), 0,
                       reinterpret_cast<hipStream_t>(hip_stream), d_msg, d_nmsg, (u32)nslots, max_msgs, d_msg_res, d_send_msg);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchSendListFromDeflatedDevice launch", e);
}

extern "C" WSFRAME_AMD_PMD_EXPORT long long websocketframeDeflateHost(
    const unsigned char* src, unsigned long long src_len, const WebsocketDeflateMsg_t* msg, unsigned int nmsg,
    unsigned long long min_len, unsigned int flags, unsigned char* dst, const unsigned long long* dst_off,
    const unsigned long long* dst_cap, WebsocketDeflateMsgRes_t* msg_res) {
    if (flags) return ws_set_msg("websocketframeDeflateHost: unknown flag");
    if ((!src && src_len) || (nmsg && (!msg || !dst_off || !dst_cap || !msg_res)))
        return ws_set_msg("websocketframeDeflateHost: invalid argument (NULL pointer)");
    return (long long)ws_deflate_list(src, src_len, msg, nmsg, min_len, dst, dst_off, dst_cap, msg_res, nullptr);
}
