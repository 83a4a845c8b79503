// ws_proto.hip — websocketframeBatchCheckProtocolDevice and websocketframeProtoStepHost
// (include/wsframe_amd_proto.h): the RFC 6455 framing and sequencing check over the descriptors
// a decode call produced, for gfx950. The rule, the run summary and its combine, and the state
// word are ws_proto.h's (one definition, host-tested).
//
// Work is divided by frames: a 32-B descriptor, one scattered header byte and, per CLOSE, two
// body bytes. The host knows no n_frames, so the plan is made on the device. The counted frames
// of all segments, laid end to end in segment order, form one list; a tile is 256 consecutive
// frames of it, one per thread. A long segment spreads over ceil(n / 256) tiles (one more when
// it starts inside a tile), short segments share a tile and a wave, an empty one costs nothing.
//   plan     one thread per segment: its frame count, the exclusive scan of the counts inside
//            its block of 256 segments and the block's sum; the segment's first-error key reset;
//   scan     one block: exclusive scan of the block sums, the total;
//   sums     a fixed grid over the tiles: every wave finds the segments of its first and last
//            frame by a 64-ary search (ballot) over the offsets, every lane its own between the
//            two; two 16-B loads fetch the descriptor; the block's segmented scan (a segment's
//            first frame forgets what came before) leaves the tile's summary;
//   combine  one block: exclusive segmented scan of the tile summaries: what each tile's first
//            segment brings along from the tiles before it;
//   verdict  the same grid and the same scan, now with the tile's carry and the connection's
//            state word in front: every frame's code (one byte store), the least error of a
//            segment (a vector atomic min on the workspace, at most one per wave and segment),
//            and the summary up to the segment's last frame;
//   finish   one thread per segment: the result record and the state word.
// Every output is written with plain vector stores; the workspace also with vector atomics.
#include <stdio.h>

#include "../../include/wsframe_amd_proto.h"
#include "ws_common.h"
#include "ws_proto.h"

#define PROTO_T 256                      // threads per block: frames per tile, segments per plan block
#define PROTO_BLOCKS_PER_CU 8            // the tile kernels' grid
#define PROTO_KEY_NONE (~0ull)           // first-error key: k << 8 | code

static_assert(sizeof(WsProtoSum) == 16 && sizeof(WebsocketProtoResult_t) == 16, "16-B records");
static_assert(WS_PROTO_ERR_TOO_BIG == WEBSOCKET_PROTO_ERR_TOO_BIG && WS_PROTO_NOT_CONSUMED == WEBSOCKET_PROTO_NOT_CONSUMED &&
                  WS_PROTO_F_WIRE_MASKED == WEBSOCKET_PROTO_WIRE_MASKED && WS_PROTO_ST_CLOSED == WEBSOCKET_PROTO_ST_CLOSED,
              "ws_proto.h and wsframe_amd_proto.h agree");

__device__ __forceinline__ WsProtoSum proto_ld(const WsProtoSum* p) {
    const u32x4 v = *gptr<u32x4>(p);
    return WsProtoSum{v.x, v.y, (u64)v.z | (u64)v.w << 32};
}
__device__ __forceinline__ void proto_st(WsProtoSum* p, const WsProtoSum& s) {
    u32x4 v;
    v.x = s.bits; v.y = s.close; v.z = (u32)s.bytes; v.w = (u32)(s.bytes >> 32);
    *gptr<u32x4>(p) = v;
}
__device__ __forceinline__ WsProtoSum proto_shfl_up(const WsProtoSum& s, int d) {
    WsProtoSum r;
    r.bits = (u32)__shfl_up((int)s.bits, d);
    r.close = (u32)__shfl_up((int)s.close, d);
    const u32 lo = (u32)__shfl_up((int)(u32)s.bytes, d), hi = (u32)__shfl_up((int)(u32)(s.bytes >> 32), d);
    r.bytes = (u64)lo | (u64)hi << 32;
    return r;
}

// Segmented scan (ws_proto_comb_seg) over the block's PROTO_T values in thread order: *excl
// takes the fold of the values before this thread, the fold of all of them is returned.
__device__ __forceinline__ WsProtoSum proto_block_scan(WsProtoSum v, WsProtoSum* wsum, WsProtoSum* excl) {
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const WsProtoSum o = proto_shfl_up(v, d);
        if (lane >= (u32)d) v = ws_proto_comb_seg(o, v);
    }
    WsProtoSum e = proto_shfl_up(v, 1);
    if (lane == 0) e = ws_proto_sum_none();
    __syncthreads();                                   // (the previous tile's readers of wsum are done)
    if (lane == 63) wsum[wv] = v;
    __syncthreads();
    WsProtoSum base = ws_proto_sum_none(), total = ws_proto_sum_none();
#pragma unroll
    for (u32 k = 0; k < PROTO_T / 64; ++k) {
        const WsProtoSum w = wsum[k];
        if (k < wv) base = ws_proto_comb_seg(base, w);
        total = ws_proto_comb_seg(total, w);
    }
    *excl = ws_proto_comb_seg(base, e);
    return total;
}

__global__ __launch_bounds__(PROTO_T) void ws_proto_plan(const WebsocketSegResult_t* res, u32 nseg, u32 max_frames,
                                                         u32* loff, u32* blocksum, u64* segkey) {
    __shared__ u32 wsum[PROTO_T / 64];
    const u32 s = blockIdx.x * PROTO_T + threadIdx.x;
    u32 n = 0;
    if (s < nseg) {
        const u32x4 r = *gptr<u32x4>(res + s);
        n = r.z < max_frames ? r.z : max_frames;
        segkey[s] = PROTO_KEY_NONE;
    }
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u32 inc = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 o = (u32)__shfl_up((int)inc, d);
        if (lane >= (u32)d) inc += o;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    u32 base = 0, total = 0;
#pragma unroll
    for (u32 k = 0; k < PROTO_T / 64; ++k) {
        if (k < wv) base += wsum[k];
        total += wsum[k];
    }
    loff[s] = base + inc - n;                          // (loff is padded to whole blocks)
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
}

// exclusive scan of the nb block sums in place; bo[nb] and head[0] take the total
__global__ __launch_bounds__(1024) void ws_proto_scan(u32* bo, u32 nb, u32* head) {
    __shared__ u32 part[1024];
    const u32 t = threadIdx.x, per = (nb + 1023) / 1024;
    const u32 lo = t * per < nb ? t * per : nb, hi = lo + per < nb ? lo + per : nb;
    u32 sum = 0;
    for (u32 k = lo; k < hi; ++k) sum += bo[k];
    part[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < 1024; d <<= 1) {
        const u32 o = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += o;
        __syncthreads();
    }
    u32 run = part[t] - sum;
    for (u32 k = lo; k < hi; ++k) {
        const u32 v = bo[k];
        bo[k] = run;
        run += v;
    }
    if (t == 1023) {
        bo[nb] = part[1023];
        head[0] = part[1023];
    }
}

// the list position of segment s's first frame (s < nseg)
__device__ __forceinline__ u32 proto_start(const u32* bo, const u32* loff, u32 s) { return bo[s / PROTO_T] + loff[s]; }

// the largest s in [0, nseg) with proto_start(s) <= f (f wave-uniform and below the total: that
// segment is not empty), by the whole wave
__device__ __forceinline__ u32 proto_search(const u32* bo, const u32* loff, u32 nseg, u32 f, u32 lane) {
    u32 lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const u32 step = (hi - lo + 63) / 64;
        const u64 idx = (u64)lo + (u64)lane * step;
        const bool le = idx < hi && proto_start(bo, loff, (u32)idx) <= f;
        const u32 cnt = (u32)__popcll(__ballot(le));   // >= 1: lane 0 probes lo
        lo += (cnt - 1) * step;
        hi = hi < lo + step ? hi : lo + step;
    }
    return lo;
}

// This thread's frame of tile t: its segment and index, the descriptor's fields, whether it is
// consumed, and its summary (with HEAD on a segment's first frame).
struct ProtoMine {
    bool valid, consumed;
    u32 s, k, n, type, fin, masked;
    u64 frame_off, data_off, datalen;
    WsProtoSum sum;
};

__device__ __forceinline__ ProtoMine proto_mine(u32 t, u32 total, const u32* bo, const u32* loff, u32 nseg, u32 max_frames,
                                                const u64* seg_off, const WebsocketFrameDesc_t* desc,
                                                const WebsocketSegResult_t* res) {
    const u32 lane = threadIdx.x & 63;
    const u32 f0 = t * PROTO_T + (threadIdx.x & ~63u), f = f0 + lane;   // (total <= 2^30: no wrap)
    ProtoMine m;
    m.valid = f < total;
    m.consumed = false;
    m.s = m.k = m.n = m.type = m.fin = m.masked = 0;
    m.frame_off = m.data_off = m.datalen = 0;
    m.sum = ws_proto_sum_none();
    if (f0 >= total) return m;                         // (wave-uniform)
    const u32 f1 = f0 + 63 < total ? f0 + 63 : total - 1;
    const u32 s0 = proto_search(bo, loff, nseg, f0, lane);
    const u32 s1 = f1 == f0 ? s0 : proto_search(bo, loff, nseg, f1, lane);
    if (!m.valid) return m;
    u32 lo = s0, hi = s1 + 1;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (proto_start(bo, loff, mid) <= f) lo = mid;
        else hi = mid;
    }
    m.s = lo;
    m.k = f - proto_start(bo, loff, lo);
    const u32x4 r = *gptr<u32x4>(res + m.s);
    m.n = r.z < max_frames ? r.z : max_frames;
    const gu32x4* const d = gptr<u32x4>(desc + ((u64)m.s * max_frames + m.k));
    const u32x4 d0 = d[0], d1 = d[1];
    m.frame_off = (u64)d0.x | (u64)d0.y << 32;
    m.data_off = (u64)d0.z | (u64)d0.w << 32;
    m.datalen = (u64)d1.x | (u64)d1.y << 32;
    const int ret = (int)d1.z;
    m.fin = d1.w & 0xFFu;
    m.type = (d1.w >> 8) & 0xFFu;
    m.masked = (d1.w >> 16) & 0xFFu;
    m.consumed = ret > 0 && m.frame_off + (u64)ret <= seg_off[m.s] + ((u64)r.x | (u64)r.y << 32);
    if (m.consumed) m.sum = ws_proto_sum_frame(m.type, m.fin, m.datalen, m.k);
    if (m.k == 0) m.sum.bits |= WS_PROTO_S_HEAD;
    return m;
}

__global__ __launch_bounds__(PROTO_T) void ws_proto_sums(const u64* seg_off, const WebsocketFrameDesc_t* desc,
                                                         const WebsocketSegResult_t* res, u32 nseg, u32 max_frames,
                                                         const u32* head, const u32* bo, const u32* loff, WsProtoSum* agg) {
    __shared__ WsProtoSum wsum[PROTO_T / 64];
    const u32 total = head[0], ntiles = (total + PROTO_T - 1) / PROTO_T;
    for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ProtoMine m = proto_mine(t, total, bo, loff, nseg, max_frames, seg_off, desc, res);
        WsProtoSum excl;
        const WsProtoSum all = proto_block_scan(m.sum, wsum, &excl);
        if (threadIdx.x == 0) proto_st(agg + t, all);
    }
}

// exclusive segmented scan of the tile summaries in place (agg[t]: what tile t's first segment
// brings along from the tiles before)
__global__ __launch_bounds__(1024) void ws_proto_combine(WsProtoSum* agg, const u32* head) {
    __shared__ WsProtoSum part[1024];
    const u32 nt = (head[0] + PROTO_T - 1) / PROTO_T;
    const u32 t = threadIdx.x, per = (nt + 1023) / 1024;
    const u32 lo = t * per < nt ? t * per : nt, hi = lo + per < nt ? lo + per : nt;
    WsProtoSum sum = ws_proto_sum_none();
    for (u32 k = lo; k < hi; ++k) sum = ws_proto_comb_seg(sum, proto_ld(agg + k));
    part[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < 1024; d <<= 1) {
        const WsProtoSum o = t >= d ? part[t - d] : ws_proto_sum_none();
        __syncthreads();
        part[t] = ws_proto_comb_seg(o, part[t]);
        __syncthreads();
    }
    WsProtoSum run = t ? part[t - 1] : ws_proto_sum_none();
    for (u32 k = lo; k < hi; ++k) {
        const WsProtoSum v = proto_ld(agg + k);
        proto_st(agg + k, run);
        run = ws_proto_comb_seg(run, v);
    }
}

__global__ __launch_bounds__(PROTO_T) void ws_proto_verdict(const unsigned char* buf, const u64* seg_off,
                                                            const WebsocketFrameDesc_t* desc, const WebsocketSegResult_t* res,
                                                            u32 nseg, u32 max_frames, WsProtoCfg cfg, const u64* state,
                                                            const u32* head, const u32* bo, const u32* loff,
                                                            const WsProtoSum* agg, unsigned char* frame_code, u64* segkey,
                                                            WsProtoSum* segfin) {
    __shared__ WsProtoSum wsum[PROTO_T / 64];
    const u32 lane = threadIdx.x & 63;
    const u32 total = head[0], ntiles = (total + PROTO_T - 1) / PROTO_T;
    for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ProtoMine m = proto_mine(t, total, bo, loff, nseg, max_frames, seg_off, desc, res);
        WsProtoSum before;
        proto_block_scan(m.sum, wsum, &before);
        u64 key = PROTO_KEY_NONE;
        if (m.valid) {
            // the frames of this segment before this one: none (its first frame), those of this
            // tile (the segment starts in it), or those with the tiles before
            if (m.k == 0) before = ws_proto_sum_none();
            else if (!(before.bits & WS_PROTO_S_HEAD)) before = ws_proto_comb(proto_ld(agg + t), before);
            before.bits &= ~WS_PROTO_S_HEAD;
            WsProtoSum mine = m.sum;
            mine.bits &= ~WS_PROTO_S_HEAD;
            if (m.k == m.n - 1) proto_st(segfin + m.s, ws_proto_comb(before, mine));
            u32 code = WS_PROTO_NOT_CONSUMED;
            if (m.consumed) {
                const u64 st = state ? state[m.s] : 0ull;
                WsProtoFrame f;
                f.type = m.type; f.fin = m.fin; f.masked = m.masked; f.datalen = m.datalen;
                f.b0 = buf[m.frame_off];
                f.close_code = 0;
                if (ws_proto_reads_close_code(m.type, m.datalen)) {
                    u32 c0 = buf[m.data_off], c1 = buf[m.data_off + 1];
                    if ((cfg.flags & WS_PROTO_F_WIRE_MASKED) && m.masked) {
                        c0 ^= buf[m.data_off - 4];
                        c1 ^= buf[m.data_off - 3];
                    }
                    f.close_code = c0 << 8 | c1;
                }
                code = ws_proto_code(ws_proto_comb(ws_proto_sum_state(st), before), (u32)((st & WS_PROTO_ST_CLOSED) != 0), f,
                                     cfg);
                if (code >= 1u && code <= 10u) key = (u64)m.k << 8 | code;
            }
            if (frame_code) frame_code[(u64)m.s * max_frames + m.k] = (unsigned char)code;
        }
        // the least error of a segment: frames are in (segment, index) order, so a wave's first
        // lane in error of each segment holds its least key
        const u64 errs = __ballot(key != PROTO_KEY_NONE);
        if (errs) {
            const u64 below = errs & ((1ull << lane) - 1);
            const int prev = below ? 63 - __builtin_clzll(below) : 0;
            const u32 sprev = (u32)__shfl((int)m.s, prev);
            if (key != PROTO_KEY_NONE && (!below || sprev != m.s)) atomicMin(&segkey[m.s], key);
        }
    }
}

__global__ __launch_bounds__(PROTO_T) void ws_proto_finish(const WebsocketSegResult_t* res, u32 nseg, u32 max_frames,
                                                           const u64* segkey, const WsProtoSum* segfin, u64* state,
                                                           WebsocketProtoResult_t* out) {
    const u32 s = blockIdx.x * PROTO_T + threadIdx.x;
    if (s >= nseg) return;
    const u32x4 r = *gptr<u32x4>(res + s);
    const u32 n = r.z < max_frames ? r.z : max_frames;
    const WsProtoSum all = n ? proto_ld(segfin + s) : ws_proto_sum_none();
    const u64 st = state ? state[s] : 0ull;
    const u64 key = segkey[s];
    const u32 code = key == PROTO_KEY_NONE ? 0u : (u32)(key & 0xFFu);
    u32x4 o;
    o.x = key == PROTO_KEY_NONE ? WS_PROTO_NONE : (u32)(key >> 8);
    o.y = code;
    o.z = ws_proto_close_status(code);
    o.w = (st & WS_PROTO_ST_CLOSED) ? WS_PROTO_NONE : all.close;
    *gptr<u32x4>(out + s) = o;
    if (state) state[s] = ws_proto_state_out(st, all);
}

static int proto_args(const char* who, unsigned int flags, unsigned int rsv_allowed) {
    static thread_local char msg[160];
    const char* why = nullptr;
    if (flags & ~WS_PROTO_F_ALL) why = "unknown flag";
    else if ((flags & WS_PROTO_F_EXPECT_MASKED) && (flags & WS_PROTO_F_EXPECT_UNMASKED))
        why = "EXPECT_MASKED and EXPECT_UNMASKED together";
    else if (rsv_allowed & ~0x70u) why = "rsv_allowed outside 0x70";
    if (!why) return 0;
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return ws_set_msg(msg);
}

extern "C" WSFRAME_AMD_PROTO_EXPORT int websocketframeBatchCheckProtocolDevice(
    const unsigned char* d_buf, const unsigned long long* d_seg_off, const WebsocketFrameDesc_t* d_desc,
    const WebsocketSegResult_t* d_res, unsigned int nseg, unsigned int max_frames, unsigned int flags,
    unsigned int rsv_allowed, unsigned long long max_message_size, unsigned long long* d_proto_state,
    unsigned char* d_frame_code, WebsocketProtoResult_t* d_proto_res, void* hip_stream) {
    if (proto_args("websocketframeBatchCheckProtocolDevice", flags, rsv_allowed)) return -1;
    if (nseg == 0) return 0;
    if (!d_buf || !d_seg_off || !d_desc || !d_res || !d_proto_res || max_frames == 0)
        return ws_set_msg("websocketframeBatchCheckProtocolDevice: invalid argument");
    if ((reinterpret_cast<uintptr_t>(d_desc) | reinterpret_cast<uintptr_t>(d_res) | reinterpret_cast<uintptr_t>(d_proto_res)) & 15)
        return ws_set_msg("websocketframeBatchCheckProtocolDevice: d_desc/d_res/d_proto_res not 16-B aligned");
    if ((reinterpret_cast<uintptr_t>(d_seg_off) | reinterpret_cast<uintptr_t>(d_proto_state)) & 7)
        return ws_set_msg("websocketframeBatchCheckProtocolDevice: d_seg_off/d_proto_state not 8-B aligned");
    const u64 nslots = (u64)nseg * max_frames;
    if (nslots > (1ull << 30)) return ws_set_msg("websocketframeBatchCheckProtocolDevice: nseg * max_frames > 2^30");
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const u32 nb = (nseg + PROTO_T - 1) / PROTO_T;
    const u32 ntmax = (u32)((nslots + PROTO_T - 1) / PROTO_T);
    // workspace (bytes, every part 16-B aligned): head[4], block offsets[nb + 1], segment offsets,
    // first-error keys, segment summaries, tile summaries
    const size_t bo_off = 16, loff_off = bo_off + (((size_t)nb + 1) * 4 + 15) / 16 * 16,
                 key_off = loff_off + (size_t)nb * PROTO_T * 4, fin_off = key_off + ((size_t)nseg * 8 + 15) / 16 * 16,
                 agg_off = fin_off + (size_t)nseg * 16, bytes = agg_off + (size_t)ntmax * 16;
    WsSlot slot;
    int rc = slot.acquire(st);
    if (rc) return rc;
    void* p = nullptr;
    if ((rc = slot.buffer(WS_BUF_PROTO, bytes, 0, &p))) return rc;
    unsigned char* const ws = reinterpret_cast<unsigned char*>(p);
    u32* const head = reinterpret_cast<u32*>(ws);
    u32* const bo = reinterpret_cast<u32*>(ws + bo_off);
    u32* const loff = reinterpret_cast<u32*>(ws + loff_off);
    u64* const segkey = reinterpret_cast<u64*>(ws + key_off);
    WsProtoSum* const segfin = reinterpret_cast<WsProtoSum*>(ws + fin_off);
    WsProtoSum* const agg = reinterpret_cast<WsProtoSum*>(ws + agg_off);
    const u32 cap = (u32)slot.cus * PROTO_BLOCKS_PER_CU, grid = ntmax < cap ? ntmax : cap;
    const WsProtoCfg cfg{flags, rsv_allowed, max_message_size};
    hipLaunchKernelGGL(ws_proto_plan, dim3(nb), dim3(PROTO_T), 0, st, d_res, nseg, max_frames, loff, bo, segkey);
    hipLaunchKernelGGL(ws_proto_scan, dim3(1), dim3(1024), 0, st, bo, nb, head);
    hipLaunchKernelGGL(ws_proto_sums, dim3(grid), dim3(PROTO_T), 0, st, d_seg_off, d_desc, d_res, nseg, max_frames, head, bo,
                       loff, agg);
    hipLaunchKernelGGL(ws_proto_combine, dim3(1), dim3(1024), 0, st, agg, head);
    hipLaunchKernelGGL(ws_proto_verdict, dim3(grid), dim3(PROTO_T), 0, st, d_buf, d_seg_off, d_desc, d_res, nseg, max_frames,
                       cfg, d_proto_state, head, bo, loff, agg, d_frame_code, segkey, segfin);
    hipLaunchKernelGGL(ws_proto_finish, dim3(nb), dim3(PROTO_T), 0, st, d_res, nseg, max_frames, segkey, segfin,
                       d_proto_state, d_proto_res);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchCheckProtocolDevice launch", e);
}

extern "C" WSFRAME_AMD_PROTO_EXPORT int websocketframeProtoStepHost(unsigned long long* state, unsigned char b0, int masked,
                                                                    unsigned long long datalen,
                                                                    const unsigned char body2[2], unsigned int flags,
                                                                    unsigned int rsv_allowed,
                                                                    unsigned long long max_message_size) {
    if (proto_args("websocketframeProtoStepHost", flags, rsv_allowed)) return -1;
    if (!state) return ws_set_msg("websocketframeProtoStepHost: invalid argument");
    WsProtoFrame f;
    f.b0 = b0; f.type = b0 & 15u; f.fin = b0 >> 7; f.masked = masked ? 1u : 0u; f.datalen = datalen;
    f.close_code = ws_proto_reads_close_code(f.type, datalen) && body2 ? (u32)body2[0] << 8 | body2[1] : 0u;
    const WsProtoCfg cfg{flags, rsv_allowed, max_message_size};
    uint64_t st = *state;
    const u32 code = ws_proto_step(&st, f, cfg);
    *state = st;
    return (int)code;
}
