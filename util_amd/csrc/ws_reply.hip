// ws_reply.hip — websocketframeBatchControlRepliesDevice and websocketframeControlRepliesHost
// (include/wsframe_amd_reply.h): PONGs, the CLOSE echo and the close status as wire bytes, from
// the descriptors a decode call produced, for gfx950. The rule, the run summary and its combine,
// the frame writer and the workspace layout are ws_reply.h's (one definition, host-tested).
//
// Work is divided by frames: the counted frames of all segments, laid end to end in segment
// order, form one list; a tile is 256 consecutive frames of it, one per thread. The plan, the
// list, the tile scan and the carries are ws_scan.h's (one definition).
//   plan     one thread per segment: its frame count, the exclusive scan of the counts inside its
//            block of 256 segments and the block's sum;
//   scan     one block: exclusive scan of the block sums, the total;
//   sums     a fixed grid over the tiles: every frame's contribution (32-B descriptor, no wire
//            byte), the block's segmented scan; the tile's summary, and for a segment's last frame
//            the fold of the segment's frames inside this tile;
//   combine  one block: exclusive segmented scan of the tile summaries;
//   segs     one thread per segment: the fold of all its frames (the tile carry in front of its
//            last tile's part), which CLOSE it sends (an ECHO reads two wire bytes), the result
//            record, the state word, its reply length; the exclusive scan of the lengths (u64)
//            inside the block of 256 segments and the block's sum;
//   offs     one block: exclusive scan of the block sums (u64), the total into d_tx_off[nseg];
//   emit     first one thread per segment: d_tx_off[s] and the CLOSE frame; then the sums grid and
//            scan again: every answered ping now knows its byte offset, and its wave copies the
//            PONGs of its lanes one after the other, lane j writing bytes j, j + 64 and j + 128
//            (any source and destination alignment; unmasking and masking go by byte position).
// Every output is written with plain vector stores.
#include <stdio.h>

#include "ws_reply.h"
#include "ws_scan.h"

#define REPLY_T 256                      // threads per block: frames per tile, segments per plan block
#define REPLY_BLOCKS_PER_CU 8            // the tile kernels' grid

static_assert(REPLY_T == WS_REPLY_T && sizeof(WsReplySum) == 32 && sizeof(WsReplyRec) == 32 &&
                  sizeof(WebsocketReplyResult_t) == 16,
              "16-B multiples");
static_assert(WEBSOCKET_REPLY_WIRE_MASKED == WEBSOCKET_PROTO_WIRE_MASKED && WS_REPLY_NONE == WEBSOCKET_PROTO_NONE,
              "wsframe_amd_reply.h and wsframe_amd_proto.h agree");

struct ReplyOps {                        // ws_scan.h's view of ws_reply.h's run summary
    typedef WsReplySum Sum;
    static constexpr u32 HEAD = WS_REPLY_S_HEAD;
    static __device__ __forceinline__ Sum none() { return ws_reply_sum_none(); }
    static __device__ __forceinline__ Sum comb(const Sum& a, const Sum& b) { return ws_reply_comb(a, b); }
    static __device__ __forceinline__ Sum comb_seg(const Sum& a, const Sum& b) { return ws_reply_comb_seg(a, b); }
};

__global__ __launch_bounds__(REPLY_T) void ws_reply_plan(const WebsocketSegResult_t* res, u32 nseg, u32 max_frames,
                                                         u32* loff, u32* blocksum) {
    __shared__ u32 wsum[REPLY_T / 64];
    const u32 s = blockIdx.x * REPLY_T + threadIdx.x;
    u64 consumed;
    const u32 n = s < nseg ? ws_seg_count(res, s, max_frames, &consumed) : 0u;
    u32 excl;
    const u32 total = ws_block_sum<REPLY_T>(n, wsum, &excl);
    loff[s] = excl;                                    // (loff is padded to whole blocks)
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
}

// exclusive scan of the nb block sums in place; bo[nb] and *total_out take the total
template <typename T>
__global__ __launch_bounds__(1024) void ws_reply_scan(T* bo, u32 nb, T* total_out) {
    __shared__ T part[1024];
    ws_offsets_scan(bo, nb, total_out, part);
}

// This thread's frame of tile t (ws_frame_mine) and its summary (with HEAD on a segment's first frame).
struct ReplyMine {
    WsFrameMine f;
    WsReplySum sum;
};

__device__ __forceinline__ ReplyMine reply_mine(u32 t, u32 total, const u32* bo, const u32* loff, u32 nseg, u32 max_frames,
                                                const u64* seg_off, const WebsocketFrameDesc_t* desc,
                                                const WebsocketSegResult_t* res, const WebsocketProtoResult_t* pres,
                                                u32 keyed) {
    ReplyMine m;
    m.f = ws_frame_mine<REPLY_T>(t, total, bo, loff, nseg, max_frames, seg_off, desc, res);
    m.sum = ws_reply_sum_none();
    if (m.f.consumed) {
        const u32 first_bad = pres ? *gptr<u32>(&pres[m.f.s].first_bad) : WS_REPLY_NONE;
        m.sum = ws_reply_sum_frame(m.f.d.type, m.f.d.fin, m.f.d.datalen, m.f.k, (u32)(m.f.k < first_bad), keyed);
    }
    if (m.f.valid && m.f.k == 0) m.sum.bits |= WS_REPLY_S_HEAD;
    return m;
}

__global__ __launch_bounds__(REPLY_T) void ws_reply_sums(const u64* seg_off, const WebsocketFrameDesc_t* desc,
                                                         const WebsocketSegResult_t* res,
                                                         const WebsocketProtoResult_t* pres, u32 nseg, u32 max_frames,
                                                         u32 keyed, const u32* head, const u32* bo, const u32* loff,
                                                         WsReplySum* agg, WsReplySum* tail) {
    __shared__ WsReplySum wsum[REPLY_T / 64];
    const u32 total = head[0], ntiles = (total + REPLY_T - 1) / REPLY_T;
    for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ReplyMine m = reply_mine(t, total, bo, loff, nseg, max_frames, seg_off, desc, res, pres, keyed);
        WsReplySum excl;
        const WsReplySum all = ws_seg_block_scan<REPLY_T, ReplyOps>(m.sum, wsum, &excl);
        if (threadIdx.x == 0) ws_st(agg + t, all);
        if (m.f.valid && m.f.k == m.f.n - 1) ws_st(tail + m.f.s, ws_reply_comb_seg(excl, m.sum));
    }
}

// exclusive segmented scan of the tile summaries in place (agg[t]: what tile t's first segment
// brings along from the tiles before)
__global__ __launch_bounds__(1024) void ws_reply_combine(WsReplySum* agg, const u32* head) {
    __shared__ WsReplySum part[1024];
    ws_seg_combine<ReplyOps>(agg, (head[0] + REPLY_T - 1) / REPLY_T, part);
}

__global__ __launch_bounds__(REPLY_T) void ws_reply_segs(const unsigned char* buf, const WebsocketFrameDesc_t* desc,
                                                         const WebsocketSegResult_t* res,
                                                         const WebsocketProtoResult_t* pres, const u32* fail, u32 nseg,
                                                         u32 max_frames, u32 flags, u32 keyed, const u32* bo, const u32* loff,
                                                         const WsReplySum* agg, const WsReplySum* tail, u32* state,
                                                         WebsocketReplyResult_t* out, WsReplyRec* rec, u64* blocksum) {
    __shared__ u64 wsum[REPLY_T / 64];
    const u32 s = blockIdx.x * REPLY_T + threadIdx.x;
    u64 bytes = 0;
    WsReplyRec r = {0ull, 0ull, 0u, WS_REPLY_NONE, 0u, 0u};
    if (s < nseg) {
        u64 consumed;
        const u32 n = ws_seg_count(res, s, max_frames, &consumed);
        const WsReplySum all =
            n ? ws_seg_fold<REPLY_T, ReplyOps>(tail + s, agg, ws_list_start<REPLY_T>(bo, loff, s), n) : ws_reply_sum_none();
        u32 first_bad = WS_REPLY_NONE, proto_status = 0;
        if (pres) {
            const u32x4 p = *gptr<u32x4>(pres + s);
            first_bad = p.x;
            proto_status = p.z;
        }
        const u32 fs = fail ? fail[s] : 0u, st = state ? state[s] : 0u;
        const u32 kind = ws_reply_close_kind(all, first_bad, fs);
        u32 status = 0, body = 2;
        if (kind == WEBSOCKET_REPLY_CLOSE_PROTOCOL) status = proto_status;
        else if (kind == WEBSOCKET_REPLY_CLOSE_CALLER) status = fs;
        else if (kind == WEBSOCKET_REPLY_CLOSE_ECHO && !(st & WEBSOCKET_REPLY_ST_CLOSE_SENT)) {
            const WsDesc d = ws_desc_ld(desc + ((u64)s * max_frames + all.close));
            if (d.datalen >= 2) status = ws_reply_echo_status(buf + d.data_off, (flags & WEBSOCKET_REPLY_WIRE_MASKED) && d.masked);
            else body = 0;
        }
        const WsReplySeg g = ws_reply_seg(all, first_bad, st, flags, keyed, kind, status, body);
        bytes = g.pong_bytes + g.close_len;
        u32x4 o;
        o.x = g.npong; o.y = g.close_kind; o.z = g.close_status; o.w = (u32)bytes;
        *gptr<u32x4>(out + s) = o;
        if (state && g.close_len) state[s] = st | WEBSOCKET_REPLY_ST_CLOSE_SENT;
        r.pong_bytes = g.pong_bytes;
        r.end = g.end;
        r.only = g.only;
        r.close = g.close_len ? g.close_len | g.close_status << 16 : 0u;
    }
    u64 excl;
    const u64 total = ws_block_sum<REPLY_T>(bytes, wsum, &excl);
    r.loc_off = excl;
    if (s < nseg) ws_st(rec + s, r);
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
}

__global__ __launch_bounds__(REPLY_T) void ws_reply_emit(const unsigned char* buf, const u64* seg_off,
                                                         const WebsocketFrameDesc_t* desc, const WebsocketSegResult_t* res,
                                                         const WebsocketProtoResult_t* pres, u32 nseg, u32 max_frames,
                                                         u32 flags, const u32* keys, const u32* head, const u32* bo,
                                                         const u32* loff, const u64* bo64, const WsReplyRec* rec,
                                                         const WsReplySum* agg, unsigned char* tx, u64 cap, u64* tx_off) {
    __shared__ WsReplySum wsum[REPLY_T / 64];
    const u32 lane = threadIdx.x & 63, keyed = keys ? 1u : 0u;
    // the segments: d_tx_off[s] and the CLOSE
    for (u64 s64 = (u64)blockIdx.x * REPLY_T + threadIdx.x; s64 < nseg; s64 += (u64)gridDim.x * REPLY_T) {
        const u32 s = (u32)s64;
        const WsReplyRec r = ws_ld(rec + s);
        const u64 base = bo64[s / REPLY_T] + r.loc_off;
        tx_off[s] = base;
        if (r.close) {
            const u32 len = r.close & 0xFFFFu, key = keyed ? keys[(u64)s * (max_frames + 1ull) + max_frames] : 0u;
            ws_reply_write(ws_reply_close(r.close >> 16, len - (keyed ? 6u : 2u), keyed, key), tx, base + r.pong_bytes, cap);
        }
    }
    // the frames: every answered ping's PONG
    const u32 total = head[0], ntiles = (total + REPLY_T - 1) / REPLY_T;
    for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ReplyMine rm = reply_mine(t, total, bo, loff, nseg, max_frames, seg_off, desc, res, pres, keyed);
        const WsFrameMine& m = rm.f;
        WsReplySum excl;
        ws_seg_block_scan<REPLY_T, ReplyOps>(rm.sum, wsum, &excl);
        bool answer = false;
        u64 off = 0;
        u32 key = 0;
        if (m.consumed) {
            const WsReplyRec r = ws_ld(rec + m.s);
            WsReplySeg g = {};
            g.end = r.end;
            g.only = r.only;
            answer = ws_reply_answers(g, flags, m.k, m.d.type, m.d.fin, m.d.datalen) != 0u;
            if (answer) {
                const WsReplySum before = ws_seg_before<ReplyOps>(excl, m.k == 0, agg + t);
                off = bo64[m.s / REPLY_T] + r.loc_off + ((flags & WEBSOCKET_REPLY_LAST_PING_ONLY) ? 0ull : before.bytes);
                if (keyed) key = keys[(u64)m.s * (max_frames + 1ull) + m.k];
            }
        }
        // the wave copies its PONGs one after the other
        const u32 wm = (flags & WEBSOCKET_REPLY_WIRE_MASKED) && m.d.masked;
        u64 todo = __ballot(answer);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const u64 o = ws_shfl(off, src), doff = ws_shfl(m.d.data_off, src);
            const u32 len = (u32)__shfl((int)(u32)m.d.datalen, src);
            const WsReplyFrame f = ws_reply_pong(buf, doff, len, (u32)__shfl((int)wm, src), keyed, (u32)__shfl((int)key, src));
            const u32 nbytes = ws_reply_frame_len(len, keyed);
            for (u32 j = lane; j < nbytes; j += 64)
                if (o + j < cap) tx[o + j] = ws_reply_byte(f, j);
        }
    }
}

static int reply_flags(const char* who, unsigned int flags, unsigned int max_frames) {
    static thread_local char msg[160];
    const char* why = nullptr;
    if (flags & ~WS_REPLY_F_ALL) why = "unknown flag";
    else if (max_frames == 0) why = "invalid argument (max_frames 0)";
    if (!why) return 0;
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return ws_set_msg(msg);
}

extern "C" WSFRAME_AMD_REPLY_EXPORT int websocketframeBatchControlRepliesDevice(
    const unsigned char* d_buf, const unsigned long long* d_seg_off, const WebsocketFrameDesc_t* d_desc,
    const WebsocketSegResult_t* d_res, unsigned int nseg, unsigned int max_frames, unsigned int flags,
    const WebsocketProtoResult_t* d_proto_res, const unsigned int* d_fail_status, const unsigned int* d_mask_key,
    unsigned int* d_reply_state, unsigned char* d_tx, unsigned long long tx_capacity, unsigned long long* d_tx_off,
    WebsocketReplyResult_t* d_reply_res, void* hip_stream) {
    if (reply_flags("websocketframeBatchControlRepliesDevice", flags, max_frames)) return -1;
    if (!d_tx_off || (!d_tx && tx_capacity) ||
        (nseg && (!d_buf || !d_seg_off || !d_desc || !d_res || !d_reply_res)))
        return ws_set_msg("websocketframeBatchControlRepliesDevice: invalid argument (NULL pointer)");
    if ((reinterpret_cast<uintptr_t>(d_desc) | reinterpret_cast<uintptr_t>(d_res) | reinterpret_cast<uintptr_t>(d_proto_res) |
         reinterpret_cast<uintptr_t>(d_reply_res)) & 15)
        return ws_set_msg("websocketframeBatchControlRepliesDevice: d_desc/d_res/d_proto_res/d_reply_res not 16-B aligned");
    if ((reinterpret_cast<uintptr_t>(d_seg_off) | reinterpret_cast<uintptr_t>(d_tx_off)) & 7)
        return ws_set_msg("websocketframeBatchControlRepliesDevice: d_seg_off/d_tx_off not 8-B aligned");
    if ((reinterpret_cast<uintptr_t>(d_fail_status) | reinterpret_cast<uintptr_t>(d_mask_key) |
         reinterpret_cast<uintptr_t>(d_reply_state)) & 3)
        return ws_set_msg("websocketframeBatchControlRepliesDevice: d_fail_status/d_mask_key/d_reply_state not 4-B aligned");
    const u64 nslots = (u64)nseg * max_frames;
    if (nslots > (1ull << 30)) return ws_set_msg("websocketframeBatchControlRepliesDevice: nseg * max_frames > 2^30");
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (nseg == 0) {
        const hipError_t e = hipMemsetAsync(d_tx_off, 0, 8, st);
        return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchControlRepliesDevice memset", e);
    }
    const WsReplyLayout L = ws_reply_layout(nseg, max_frames);
    WsSlot slot;
    int rc = slot.acquire(st);
    if (rc) return rc;
    void* p = nullptr;
    if ((rc = slot.buffer(WS_BUF_REPLY, L.bytes, 0, &p))) return rc;
    unsigned char* const ws = reinterpret_cast<unsigned char*>(p);
    u32* const head = reinterpret_cast<u32*>(ws);
    u32* const bo = reinterpret_cast<u32*>(ws + L.bo);
    u32* const loff = reinterpret_cast<u32*>(ws + L.loff);
    u64* const bo64 = reinterpret_cast<u64*>(ws + L.bo64);
    WsReplyRec* const rec = reinterpret_cast<WsReplyRec*>(ws + L.rec);
    WsReplySum* const tail = reinterpret_cast<WsReplySum*>(ws + L.tail);
    WsReplySum* const agg = reinterpret_cast<WsReplySum*>(ws + L.agg);
    const u32 cap = (u32)slot.cus * REPLY_BLOCKS_PER_CU, grid = L.ntmax < cap ? L.ntmax : cap;
    const u32 keyed = d_mask_key ? 1u : 0u;
    u64* const tx_off = reinterpret_cast<u64*>(d_tx_off);
    hipLaunchKernelGGL(ws_reply_plan, dim3(L.nb), dim3(REPLY_T), 0, st, d_res, nseg, max_frames, loff, bo);
    hipLaunchKernelGGL(ws_reply_scan<u32>, dim3(1), dim3(1024), 0, st, bo, L.nb, head);
    hipLaunchKernelGGL(ws_reply_sums, dim3(grid), dim3(REPLY_T), 0, st, reinterpret_cast<const u64*>(d_seg_off), d_desc, d_res,
                       d_proto_res, nseg, max_frames, keyed, head, bo, loff, agg, tail);
    hipLaunchKernelGGL(ws_reply_combine, dim3(1), dim3(1024), 0, st, agg, head);
    hipLaunchKernelGGL(ws_reply_segs, dim3(L.nb), dim3(REPLY_T), 0, st, d_buf, d_desc, d_res, d_proto_res, d_fail_status, nseg,
                       max_frames, flags, keyed, bo, loff, agg, tail, d_reply_state, d_reply_res, rec, bo64);
    hipLaunchKernelGGL(ws_reply_scan<u64>, dim3(1), dim3(1024), 0, st, bo64, L.nb, tx_off + nseg);
    hipLaunchKernelGGL(ws_reply_emit, dim3(grid), dim3(REPLY_T), 0, st, d_buf, reinterpret_cast<const u64*>(d_seg_off), d_desc,
                       d_res, d_proto_res, nseg, max_frames, flags, d_mask_key, head, bo, loff, bo64, rec, agg, d_tx,
                       (u64)tx_capacity, tx_off);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchControlRepliesDevice launch", e);
}

extern "C" WSFRAME_AMD_REPLY_EXPORT long long websocketframeControlRepliesHost(
    const unsigned char* buf, unsigned long long seg_off, const WebsocketFrameDesc_t* desc, const WebsocketSegResult_t* res,
    unsigned int max_frames, unsigned int flags, const WebsocketProtoResult_t* proto_res, unsigned int fail_status,
    const unsigned int* mask_key, unsigned int* state, unsigned char* tx, unsigned long long tx_capacity,
    WebsocketReplyResult_t* out) {
    if (reply_flags("websocketframeControlRepliesHost", flags, max_frames)) return -1;
    if (!buf || !desc || !res || !out || (!tx && tx_capacity))
        return ws_set_msg("websocketframeControlRepliesHost: invalid argument (NULL pointer)");
    return (long long)ws_reply_segment(buf, seg_off, desc, res, max_frames, flags, proto_res, fail_status, mask_key, state, tx,
                                       tx_capacity, out);
}
