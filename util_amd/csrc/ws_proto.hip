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
// The plan, the list, the tile scan and the carry are ws_scan.h's (one definition):
//   plan     one thread per segment: its frame count, the exclusive scan of the counts inside
//            its block of 256 segments and the block's sum; the segment's first-error key reset;
//   scan     one block: exclusive scan of the block sums, the total;
//   sums     a fixed grid over the tiles: every lane finds its frame's segment and fetches the
//            descriptor; the block's segmented scan (a segment's first frame forgets what came
//            before) leaves the tile's summary;
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
#include "ws_proto.h"
#include "ws_scan.h"

#define PROTO_T 256                      // threads per block: frames per tile, segments per plan block
#define PROTO_BLOCKS_PER_CU 8            // the tile kernels' grid
#define PROTO_KEY_NONE (~0ull)           // first-error key: k << 8 | code

static_assert(sizeof(WsProtoSum) == 16 && sizeof(WebsocketProtoResult_t) == 16, "16-B records");
static_assert(WS_PROTO_ERR_TOO_BIG == WEBSOCKET_PROTO_ERR_TOO_BIG && WS_PROTO_NOT_CONSUMED == WEBSOCKET_PROTO_NOT_CONSUMED &&
                  WS_PROTO_F_WIRE_MASKED == WEBSOCKET_PROTO_WIRE_MASKED && WS_PROTO_ST_CLOSED == WEBSOCKET_PROTO_ST_CLOSED,
              "ws_proto.h and wsframe_amd_proto.h agree");

struct ProtoOps {                        // ws_scan.h's view of ws_proto.h's run summary
    typedef WsProtoSum Sum;
    static constexpr u32 HEAD = WS_PROTO_S_HEAD;
    static __device__ __forceinline__ Sum none() { return ws_proto_sum_none(); }
    static __device__ __forceinline__ Sum comb(const Sum& a, const Sum& b) { return ws_proto_comb(a, b); }
    static __device__ __forceinline__ Sum comb_seg(const Sum& a, const Sum& b) { return ws_proto_comb_seg(a, b); }
};

__global__ __launch_bounds__(PROTO_T) void ws_proto_plan(const WebsocketSegResult_t* res, u32 nseg, u32 max_frames,
                                                         u32* loff, u32* blocksum, u64* segkey) {
    __shared__ u32 wsum[PROTO_T / 64];
    const u32 s = blockIdx.x * PROTO_T + threadIdx.x;
    u32 n = 0;
    if (s < nseg) {
        u64 consumed;
        n = ws_seg_count(res, s, max_frames, &consumed);
        segkey[s] = PROTO_KEY_NONE;
    }
    u32 excl;
    const u32 total = ws_block_sum<PROTO_T>(n, wsum, &excl);
    loff[s] = excl;                                    // (loff is padded to whole blocks)
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
}

// exclusive scan of the nb block sums in place; bo[nb] and head[0] take the total
__global__ __launch_bounds__(1024) void ws_proto_scan(u32* bo, u32 nb, u32* head) {
    __shared__ u32 part[1024];
    ws_offsets_scan(bo, nb, head, part);
}

// This thread's frame of tile t (ws_frame_mine) and its summary (with HEAD on a segment's first frame).
struct ProtoMine {
    WsFrameMine f;
    WsProtoSum sum;
};

__device__ __forceinline__ ProtoMine proto_mine(u32 t, u32 total, const u32* bo, const u32* loff, u32 nseg, u32 max_frames,
                                                const u64* seg_off, const WebsocketFrameDesc_t* desc,
                                                const WebsocketSegResult_t* res) {
    ProtoMine m;
    m.f = ws_frame_mine<PROTO_T>(t, total, bo, loff, nseg, max_frames, seg_off, desc, res);
    m.sum = ws_proto_sum_none();
    if (m.f.consumed) m.sum = ws_proto_sum_frame(m.f.d.type, m.f.d.fin, m.f.d.datalen, m.f.k);
    if (m.f.valid && m.f.k == 0) m.sum.bits |= WS_PROTO_S_HEAD;
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
        const WsProtoSum all = ws_seg_block_scan<PROTO_T, ProtoOps>(m.sum, wsum, &excl);
        if (threadIdx.x == 0) ws_st(agg + t, all);
    }
}

// exclusive segmented scan of the tile summaries in place (agg[t]: what tile t's first segment
// brings along from the tiles before)
__global__ __launch_bounds__(1024) void ws_proto_combine(WsProtoSum* agg, const u32* head) {
    __shared__ WsProtoSum part[1024];
    ws_seg_combine<ProtoOps>(agg, (head[0] + PROTO_T - 1) / PROTO_T, part);
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
        const ProtoMine pm = proto_mine(t, total, bo, loff, nseg, max_frames, seg_off, desc, res);
        const WsFrameMine& m = pm.f;
        WsProtoSum excl;
        ws_seg_block_scan<PROTO_T, ProtoOps>(pm.sum, wsum, &excl);
        u64 key = PROTO_KEY_NONE;
        if (m.valid) {
            WsProtoSum before = ws_seg_before<ProtoOps>(excl, m.k == 0, agg + t);
            before.bits &= ~WS_PROTO_S_HEAD;
            WsProtoSum mine = pm.sum;
            mine.bits &= ~WS_PROTO_S_HEAD;
            if (m.k == m.n - 1) ws_st(segfin + m.s, ws_proto_comb(before, mine));
            u32 code = WS_PROTO_NOT_CONSUMED;
            if (m.consumed) {
                const u64 st = state ? state[m.s] : 0ull;
                WsProtoFrame f;
                f.type = m.d.type; f.fin = m.d.fin; f.masked = m.d.masked; f.datalen = m.d.datalen;
                f.b0 = buf[m.d.frame_off];
                f.close_code = 0;
                if (ws_proto_reads_close_code(m.d.type, m.d.datalen)) {
                    u32 c0 = buf[m.d.data_off], c1 = buf[m.d.data_off + 1];
                    if ((cfg.flags & WS_PROTO_F_WIRE_MASKED) && m.d.masked) {
                        c0 ^= buf[m.d.data_off - 4];
                        c1 ^= buf[m.d.data_off - 3];
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
    u64 consumed;
    const u32 n = ws_seg_count(res, s, max_frames, &consumed);
    const WsProtoSum all = n ? ws_ld(segfin + s) : ws_proto_sum_none();
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
