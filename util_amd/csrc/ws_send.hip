// ws_send.hip — websocketframeBatchSendDevice, websocketframeBatchSendListFromMessagesDevice and
// websocketframeSendHost (include/wsframe_amd_send.h), and their ext twins that can set RSV1
// (include/wsframe_amd_compress.h: the same kernels, one bit in the record): every connection's messages fragmented,
// framed and packed into its wire bytes, for gfx950. The rule, the closed-form lengths, the byte
// function, the slot summary and its combine, the record and the workspace layout are ws_send.h's
// (one definition, host-tested). No per-frame record exists anywhere: a frame is found inside its
// message by division by the frame stride.
//
// The message slots of all connections, s * max_msgs + i, form one list; a tile is 256 consecutive
// slots of it, one per thread (the tile scan, the carries and the offsets scan are ws_scan.h's, one
// definition; no atomics).
//   sums     a fixed grid over the tiles: every slot's summary (its entry validated, its wire
//            length and frame count in closed form), the block's segmented scan; the tile's
//            summary, and for a connection's last slot the fold of its slots inside this tile;
//   combine  one block: exclusive segmented scan of the tile summaries;
//   segs     one thread per connection: the fold of all its slots (the tile carry in front of its
//            last tile's part), its result record, its length (0 when it failed); the exclusive
//            scan of the lengths (u64) inside the block of 256 connections and the block's sum;
//   offs     one block: exclusive scan of the block sums (u64), the total into d_tx_off[nseg];
//   recs     the sums grid and scan again: every slot now knows its first wire byte; its record,
//            d_tx_off, d_msg_tx_off, and for every 16 KiB piece of d_tx whose first byte the
//            message holds, the piece's pointer to this slot;
//   emit     one-shot 256-thread blocks, one per 16 KiB piece (the grid is sized from tx_capacity;
//            blocks past min(total, capacity) exit at once), 4 x 16 B per lane. A lane finds the
//            record that holds its chunk's first byte by bisection between its piece's pointer and
//            the next one (the records' offsets staged in LDS when at most 2048 lie between), the
//            frame by one division. A chunk wholly inside one payload is one unaligned 16-B source
//            load, XOR with the key rotated to the chunk's phase and an aligned non-temporal 16-B
//            store; every other chunk (header bytes, frame, message and connection edges, the end
//            of the total, the capacity cut, d_tx's own phase) is built a run at a time, walking on
//            through the records: ws_send_locate finds the frame (the one division), header and
//            key bytes come from ws_send_frame_byte — the two halves of ws_send_byte — and a
//            payload run is one 16-B source window cut to the run; exactly those bytes are stored.
// Every output is written with plain vector stores.
#include <stdio.h>

#include "ws_scan.h"
#include "ws_send.h"
#include "../../include/wsframe_amd_compress.h"   // the ext entry points (RSV1): declared there, built here

#define SEND_T 256                       // threads per block: slots per tile, connections per segs block
#define SEND_BLOCKS_PER_CU 8             // the tile kernels' grid
#define SEND_U 4                         // 16-B chunks per lane in emit
#define SEND_PIECE (1u << WS_SEND_PIECE_SHIFT)
#define SEND_LDS_RECS 2048u              // record offsets staged per piece (8 KiB of LDS)

static_assert(SEND_T == WS_SEND_T && SEND_T * SEND_U * 16 == SEND_PIECE, "a block covers one piece");
static_assert(WS_SEND_F_RSV1 == WEBSOCKET_SEND_FLAG_RSV1 && WS_SEND_T_RSV1 == WEBSOCKET_SEND_TYPE_RSV1, "ws_send.h restates the public bits");
static_assert(sizeof(WsSendSum) == 32 && sizeof(WsSendRec) == 48 && sizeof(WebsocketSendResult_t) == 32 &&
                  sizeof(WebsocketSendMsg_t) == 24,
              "record sizes");

typedef u32x4 __attribute__((aligned(1))) u32x4u;

struct SendOps {                         // ws_scan.h's view of ws_send.h's slot summary
    typedef WsSendSum Sum;
    static constexpr u32 HEAD = WS_SEND_S_HEAD;
    static __device__ __forceinline__ Sum none() { return ws_send_sum_none(); }
    static __device__ __forceinline__ Sum comb(const Sum& a, const Sum& b) { return ws_send_comb(a, b); }
    static __device__ __forceinline__ Sum comb_seg(const Sum& a, const Sum& b) { return ws_send_comb_seg(a, b); }
};

__device__ __forceinline__ u64 rec_tx_off(const WsSendRec* p) { return *gptr<u64>(p); }

// This thread's slot of tile t: its connection and index, the connection's count, fragment size
// and shard, the entry, and its summary (with HEAD on a connection's first slot).
struct SendMine {
    bool valid, live;             // a slot of the list; an entry of its connection (i < n)
    u32 q, s, i, shard, key;
    WebsocketSendMsg_t m;
    WsSendSum sum;
};

__device__ __forceinline__ SendMine send_mine(u32 t, u32 nslots, u32 max_msgs, u64 src_len, const WebsocketSendMsg_t* msg,
                                              const u32* nmsg, const u32* frag, const u32* keys) {
    SendMine m;
    m.q = t * SEND_T + threadIdx.x;                    // (nslots <= 2^30: no wrap)
    m.valid = m.q < nslots;
    m.live = false;
    m.s = m.i = m.shard = m.key = 0;
    m.m.src_off = m.m.len = 0;
    m.m.type = WEBSOCKET_SEND_SKIP;
    m.m.reserved = 0;
    m.sum = ws_send_sum_none();
    if (!m.valid) return m;
    m.s = m.q / max_msgs;
    m.i = m.q - m.s * max_msgs;
    const u32 cnt = *gptr<u32>(nmsg + m.s), n = cnt < max_msgs ? cnt : max_msgs;
    const u32 F = frag ? *gptr<u32>(frag + m.s) : WEBSOCKET_SEND_FRAG_DEFAULT, role = keys ? 1u : 0u;
    m.shard = ws_send_shard(F, role);
    m.live = m.i < n;
    if (m.live) {
        const gu64* const g = gptr<u64>(msg + m.q);
        const u64 w = g[2];
        m.m.src_off = g[0];
        m.m.len = g[1];
        m.m.type = (u32)w;
        if (keys) m.key = *gptr<u32>(keys + m.q);
        m.sum = ws_send_sum_msg(m.m, m.i, src_len, F, role);
    }
    if (m.i == 0) m.sum.bits |= WS_SEND_S_HEAD;
    return m;
}

__global__ __launch_bounds__(SEND_T) void ws_send_sums(const WebsocketSendMsg_t* msg, const u32* nmsg, const u32* frag,
                                                       const u32* keys, u32 nslots, u32 max_msgs, u64 src_len, u32 ntiles,
                                                       WsSendSum* agg, WsSendSum* tail) {
    __shared__ WsSendSum wsum[SEND_T / 64];
    for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const SendMine m = send_mine(t, nslots, max_msgs, src_len, msg, nmsg, frag, keys);
        WsSendSum excl;
        const WsSendSum all = ws_seg_block_scan<SEND_T, SendOps>(m.sum, wsum, &excl);
        if (threadIdx.x == 0) ws_st(agg + t, all);
        if (m.valid && m.i == max_msgs - 1) ws_st(tail + m.s, ws_send_comb_seg(excl, m.sum));
    }
}

// exclusive segmented scan of the tile summaries in place (agg[t]: what tile t's first connection
// brings along from the tiles before)
__global__ __launch_bounds__(1024) void ws_send_combine(WsSendSum* agg, u32 nt) {
    __shared__ WsSendSum part[1024];
    ws_seg_combine<SendOps>(agg, nt, part);
}

__global__ __launch_bounds__(SEND_T) void ws_send_segs(u32 nseg, u32 max_msgs, const WsSendSum* agg, const WsSendSum* tail,
                                                       WebsocketSendResult_t* out, u64* loc, u64* blocksum) {
    __shared__ u64 wsum[SEND_T / 64];
    const u32 s = blockIdx.x * SEND_T + threadIdx.x;
    u64 bytes = 0;
    if (s < nseg) {
        const WebsocketSendResult_t r = ws_send_result(ws_seg_fold<SEND_T, SendOps>(tail + s, agg, (u64)s * max_msgs, max_msgs));
        bytes = r.tx_len;
        ws_st(out + s, r);
    }
    u64 excl;
    const u64 total = ws_block_sum<SEND_T>(bytes, wsum, &excl);
    loc[s] = excl;                                     // (loc is padded to whole blocks)
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
}

// exclusive scan of the nb block sums in place; bo[nb] and *total_out take the total
__global__ __launch_bounds__(1024) void ws_send_offs(u64* bo, u32 nb, u64* total_out) {
    __shared__ u64 part[1024];
    ws_offsets_scan(bo, nb, total_out, part);
}

__global__ __launch_bounds__(SEND_T) void ws_send_recs(const WebsocketSendMsg_t* msg, const u32* nmsg, const u32* frag,
                                                       const u32* keys, u32 nseg, u32 nslots, u32 max_msgs, u64 src_len,
                                                       u32 ntiles, const WsSendSum* agg, const WebsocketSendResult_t* res,
                                                       const u64* bo64, const u64* loc, u64 cap, u32 lead, u32 flags,
                                                       WsSendRec* rec, u32* ptr, u64* tx_off, u64* msg_tx_off) {
    __shared__ WsSendSum wsum[SEND_T / 64];
    const u64 total = tx_off[nseg], limit = total < cap ? total : cap;
    const u64 np = ws_send_pieces(limit, lead);
    for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const SendMine m = send_mine(t, nslots, max_msgs, src_len, msg, nmsg, frag, keys);
        WsSendSum excl;
        ws_seg_block_scan<SEND_T, SendOps>(m.sum, wsum, &excl);
        if (!m.valid) continue;
        const WsSendSum before = ws_seg_before<SendOps>(excl, m.i == 0, agg + t);
        const bool ok = *gptr<u32>(&res[m.s].status) == WEBSOCKET_SEND_OK;
        const u64 base = bo64[m.s / SEND_T] + loc[m.s];
        WsSendRec r;
        r.tx_off = base + (ok ? before.bytes : 0ull);
        r.src_off = m.m.src_off;
        r.len = m.m.len;
        r.wire = ok && m.sum.nmsg ? m.sum.bytes : 0ull;
        r.shard = m.shard;
        r.key = m.key;
        r.type = ws_send_rec_type(m.m.type, flags);
        r.role = keys ? 1u : 0u;
        ws_st(rec + m.q, r);
        if (m.i == 0) tx_off[m.s] = base;
        if (msg_tx_off && m.live) msg_tx_off[m.q] = r.tx_off;
        if (r.wire && r.tx_off < limit) {
            // the pieces whose first byte (of d_tx for piece 0) this message holds
            const u64 end = r.tx_off + r.wire;
            u64 p = r.tx_off ? (r.tx_off + lead + SEND_PIECE - 1) >> WS_SEND_PIECE_SHIFT : 0ull;
            const u64 pe = (end - 1 + lead) >> WS_SEND_PIECE_SHIFT;
            for (; p <= pe && p < np; ++p) ptr[p] = m.q;
        }
    }
}

// the frame of message r that holds wire position p, when [p, p + 16) lies inside its payload:
// *k takes the payload byte p stands for (counted from the message's body), *fk the frame's key
// rotated to the chunk's phase: chunk byte i takes the key byte of frame body byte (q - hl) + i
__device__ __forceinline__ bool send_interior(const WsSendRec& r, u64 p, u64* k, u32* fk) {
    if (r.len < 16 || p >= r.wire || p + 16 > r.wire) return false;
    const u32 stride = ws_send_stride(r.shard, r.role);
    const u64 j = (p >> 32) ? p / stride : (u64)((u32)p / stride);
    const u32 q = (u32)(p - j * stride);
    const u64 body0 = j * r.shard, left = r.len - body0;
    const u32 flen = left < r.shard ? (u32)left : r.shard, hl = ws_send_hdr_len(flen, r.role);
    if (q < hl || (u64)q + 16 > (u64)hl + flen) return false;
    *k = body0 + (q - hl);
    const u32 key = ws_send_frag_key(r.key, j), sh = 8u * ((q - hl) & 3u);
    *fk = sh ? (key >> sh) | (key << (32u - sh)) : key;
    return true;
}

__global__ __launch_bounds__(SEND_T) void ws_send_emit(const unsigned char* src, u64 src_len, u32 nseg, u32 nslots, const WsSendRec* rec,
                                                       const u32* ptr, const u64* tx_off, unsigned char* tx, u64 cap,
                                                       u32 lead) {
    __shared__ u32 rel[SEND_LDS_RECS];
    const u64 total = tx_off[nseg], limit = total < cap ? total : cap;
    const u64 np = ws_send_pieces(limit, lead), p = blockIdx.x;
    if (p >= np) return;
    // the records between this piece's pointer and the next one's (the last piece: the list's end)
    // (a pointer is never past the list: the clamps only keep a wrong one from leaving the records)
    const u32 lo = ptr[p] < nslots ? ptr[p] : nslots - 1;
    const u32 nx = p + 1 < np && ptr[p + 1] < nslots ? ptr[p + 1] : nslots - 1, hi = nx > lo ? nx : lo, nrec = hi - lo + 1;
    const u64 y0 = p << WS_SEND_PIECE_SHIFT;               // positions y count from d_tx - lead: 16-B aligned
    const bool staged = nrec <= SEND_LDS_RECS;
    if (staged) {
        for (u32 k = threadIdx.x; k < nrec; k += SEND_T) {
            const u64 y = rec_tx_off(rec + lo + k) + lead;
            rel[k] = y <= y0 ? 0u : (y - y0 < SEND_PIECE ? (u32)(y - y0) : SEND_PIECE);
        }
        __syncthreads();
    }
    unsigned char* const txb = tx - lead;
#pragma unroll 1
    for (u32 u = 0; u < SEND_U; ++u) {
        const u64 y = y0 + (u64)(u * SEND_T + threadIdx.x) * 16;
        if (y + 16 <= lead || y >= limit + lead) continue;  // no byte of d_tx[0, limit) in this chunk
        const u64 xs = y < lead ? 0ull : y - lead;          // the chunk's first byte that is one of d_tx's
        // the last record of [lo, hi] that starts at or before xs: it holds xs
        u32 a = 0, b = nrec;
        if (staged) {
            const u32 want = (u32)(xs + lead - y0);
            while (b - a > 1) {
                const u32 mid = a + (b - a) / 2;
                if (rel[mid] <= want) a = mid;
                else b = mid;
            }
        } else {
            while (b - a > 1) {
                const u32 mid = a + (b - a) / 2;
                if (rec_tx_off(rec + lo + mid) <= xs) a = mid;
                else b = mid;
            }
        }
        u32 j = lo + a;
        WsSendRec r = ws_ld(rec + j);
        u64 k;
        u32 fk;
        if (y >= lead && y + 16 <= limit + lead && send_interior(r, xs - r.tx_off, &k, &fk)) {
            u32x4 v = *reinterpret_cast<const WS_GLOBAL u32x4u*>(reinterpret_cast<uintptr_t>(src + r.src_off + k));
            if (r.role) {
                v.x ^= fk; v.y ^= fk; v.z ^= fk; v.w ^= fk;
            }
            __builtin_nontemporal_store(v, gptr<u32x4>(txb + y));
            continue;
        }
        // the exact path, a run at a time: header and key bytes from ws_send_frame_byte, a payload run
        // as one unaligned 16-B window of the source (where the window lies inside d_src) cut to
        // the run's bytes, else byte by byte
        u32 w0 = 0, w1 = 0, w2 = 0, w3 = 0, cov = 0;
        u32 i = y < lead ? lead - (u32)y : 0u;
#pragma unroll 1
        while (i < 16) {
            const u64 x = y + i - lead;
            if (x >= limit) break;
            while (x >= r.tx_off + r.wire && j + 1 < nslots) r = ws_ld(rec + ++j);   // (x < total: a record holds it)
            if (x - r.tx_off >= r.wire) break;
            const WsSendLoc f = ws_send_locate(r, x - r.tx_off);
            const u32 hx = f.hl + (r.role ? 4u : 0u);
            const u64 room = limit - x;
            u32 run = 16u - i;
            if (room < run) run = (u32)room;
            u32 b0 = 0, b1 = 0, b2 = 0, b3 = 0;            // the run's bytes at their place in the chunk
            if (f.q < hx) {
                if (hx - f.q < run) run = hx - f.q;
                for (u32 t = 0; t < run; ++t) {
                    const u32 v = (u32)ws_send_frame_byte(r, src, f, f.q + t) << (8u * ((i + t) & 3u)), d = (i + t) >> 2;
                    b0 |= d == 0 ? v : 0u; b1 |= d == 1 ? v : 0u; b2 |= d == 2 ? v : 0u; b3 |= d == 3 ? v : 0u;
                }
            } else {
                const u32 k = f.q - hx;
                if (f.flen - k < run) run = f.flen - k;
                const u64 at = r.src_off + f.body0 + k;    // the run's first source byte
                if (at >= i && at - i + 16 <= src_len) {
                    u32x4 v = *reinterpret_cast<const WS_GLOBAL u32x4u*>(reinterpret_cast<uintptr_t>(src + (at - i)));
                    if (r.role) {                          // chunk byte c takes the key byte of body byte k + c - i
                        const u32 key = ws_send_frag_key(r.key, f.j), sh = 8u * ((k - i) & 3u);
                        const u32 rk = sh ? (key >> sh) | (key << (32u - sh)) : key;
                        v.x ^= rk; v.y ^= rk; v.z ^= rk; v.w ^= rk;
                    }
                    const u32 bits = (0xFFFFu >> (16u - (i + run))) & (0xFFFFu << i);
                    b0 = v.x & nib_to_bytemask(bits & 15u);
                    b1 = v.y & nib_to_bytemask((bits >> 4) & 15u);
                    b2 = v.z & nib_to_bytemask((bits >> 8) & 15u);
                    b3 = v.w & nib_to_bytemask(bits >> 12);
                } else {
                    for (u32 t = 0; t < run; ++t) {
                        const u32 v = (u32)ws_send_frame_byte(r, src, f, f.q + t) << (8u * ((i + t) & 3u)), d = (i + t) >> 2;
                        b0 |= d == 0 ? v : 0u; b1 |= d == 1 ? v : 0u; b2 |= d == 2 ? v : 0u; b3 |= d == 3 ? v : 0u;
                    }
                }
            }
            w0 |= b0; w1 |= b1; w2 |= b2; w3 |= b3;
            cov |= (0xFFFFu >> (16u - (i + run))) & (0xFFFFu << i);
            i += run;
        }
        u32x4 w;
        w.x = w0; w.y = w1; w.z = w2; w.w = w3;
        if (cov == 0xFFFFu) *gptr<u32x4>(txb + y) = w;
        else ws_store_bytes(gptr<unsigned char>(txb + y), w, cov);
    }
}

// the echo's send list: slot (s, i) from reassembly's message i of connection s
__global__ __launch_bounds__(SEND_T) void ws_send_list(const WebsocketFrameDesc_t* desc, const WebsocketMsgDesc_t* msg,
                                                       const u32* nmsg, u32 nslots, u32 max_frames, WebsocketSendMsg_t* out) {
    const u64 q64 = (u64)blockIdx.x * SEND_T + threadIdx.x;
    if (q64 >= nslots) return;
    const u32 q = (u32)q64, s = q / max_frames, i = q - s * max_frames;
    const u32 cnt = *gptr<u32>(nmsg + s);
    if (i >= (cnt < max_frames ? cnt : max_frames)) return;
    const gu32x4* const g = gptr<u32x4>(msg + q);
    const u32x4 a = g[0], b = g[1];                        // out_off, len | first_frame, n_frames, complete, continued
    u32 type = WEBSOCKET_SEND_SKIP;
    if (b.z && !b.w && b.x < max_frames) {
        const u32 t = (gptr<u32x4>(desc + ((u64)s * max_frames + b.x))[1].w >> 8) & 0xFFu;
        if (t == 1u || t == 2u) type = t;
    }
    const bool send = type != WEBSOCKET_SEND_SKIP;
    gu64* const o = gptr<u64>(out + q);
    o[0] = send ? (u64)a.x | (u64)a.y << 32 : 0ull;
    o[1] = send ? (u64)a.z | (u64)a.w << 32 : 0ull;
    o[2] = (u64)type;
}

// the batch send behind both entry points: `who` names the caller in error texts, flags is 0 or
// WEBSOCKET_SEND_FLAG_RSV1 (checked by the caller)
static int send_batch(const char* who, const unsigned char* d_src, unsigned long long src_len, const WebsocketSendMsg_t* d_msg,
                      const unsigned int* d_nmsg, unsigned int nseg, unsigned int max_msgs, const unsigned int* d_frag_size,
                      const unsigned int* d_mask_key, unsigned int flags, unsigned char* d_tx, unsigned long long tx_capacity,
                      unsigned long long* d_tx_off, unsigned long long* d_msg_tx_off, WebsocketSendResult_t* d_send_res,
                      void* hip_stream) {
    char text[160];
    auto fail = [&](const char* what) {
        snprintf(text, sizeof text, "%s: %s", who, what);
        return ws_set_msg(text);
    };
    if (max_msgs == 0) return fail("invalid argument (max_msgs 0)");
    if (!d_tx_off || (!d_tx && tx_capacity) || (nseg && (!d_src || !d_msg || !d_nmsg || !d_send_res)))
        return fail("invalid argument (NULL pointer)");
    if (reinterpret_cast<uintptr_t>(d_send_res) & 15)
        return fail("d_send_res not 16-B aligned");
    if ((reinterpret_cast<uintptr_t>(d_msg) | reinterpret_cast<uintptr_t>(d_tx_off) | reinterpret_cast<uintptr_t>(d_msg_tx_off)) & 7)
        return fail("d_msg/d_tx_off/d_msg_tx_off not 8-B aligned");
    if ((reinterpret_cast<uintptr_t>(d_nmsg) | reinterpret_cast<uintptr_t>(d_frag_size) | reinterpret_cast<uintptr_t>(d_mask_key)) & 3)
        return fail("d_nmsg/d_frag_size/d_mask_key not 4-B aligned");
    if (src_len > WS_SEND_SRC_MAX) return fail("src_len > 2^56");
    if (tx_capacity > (1ull << 44)) return fail("tx_capacity > 2^44");
    const u64 nslots64 = (u64)nseg * max_msgs;
    if (nslots64 > (1ull << 30)) return fail("nseg * max_msgs > 2^30");
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (nseg == 0) {
        const hipError_t e = hipMemsetAsync(d_tx_off, 0, 8, st);
        return e == hipSuccess ? 0 : (snprintf(text, sizeof text, "%s memset", who), ws_set_err(text, e));
    }
    const u32 nslots = (u32)nslots64;
    const WsSendLayout L = ws_send_layout(nseg, max_msgs, tx_capacity);
    WsSlot slot;
    int rc = slot.acquire(st);
    if (rc) return rc;
    void* p = nullptr;
    if ((rc = slot.buffer(WS_BUF_SEND, L.bytes, 0, &p))) return rc;
    unsigned char* const ws = reinterpret_cast<unsigned char*>(p);
    u64* const bo64 = reinterpret_cast<u64*>(ws + L.bo64);
    u64* const loc = reinterpret_cast<u64*>(ws + L.loc);
    WsSendSum* const tail = reinterpret_cast<WsSendSum*>(ws + L.tail);
    WsSendSum* const agg = reinterpret_cast<WsSendSum*>(ws + L.agg);
    WsSendRec* const rec = reinterpret_cast<WsSendRec*>(ws + L.rec);
    u32* const ptr = reinterpret_cast<u32*>(ws + L.ptr);
    const u32 gcap = (u32)slot.cus * SEND_BLOCKS_PER_CU, grid = L.ntiles < gcap ? L.ntiles : gcap;
    const u32 lead = (u32)(reinterpret_cast<uintptr_t>(d_tx) & 15);
    u64* const tx_off = reinterpret_cast<u64*>(d_tx_off);
    hipLaunchKernelGGL(ws_send_sums, dim3(grid), dim3(SEND_T), 0, st, d_msg, d_nmsg, d_frag_size, d_mask_key, nslots, max_msgs,
                       (u64)src_len, L.ntiles, agg, tail);
    hipLaunchKernelGGL(ws_send_combine, dim3(1), dim3(1024), 0, st, agg, L.ntiles);
    hipLaunchKernelGGL(ws_send_segs, dim3(L.nb), dim3(SEND_T), 0, st, nseg, max_msgs, agg, tail, d_send_res, loc, bo64);
    hipLaunchKernelGGL(ws_send_offs, dim3(1), dim3(1024), 0, st, bo64, L.nb, tx_off + nseg);
    hipLaunchKernelGGL(ws_send_recs, dim3(grid), dim3(SEND_T), 0, st, d_msg, d_nmsg, d_frag_size, d_mask_key, nseg, nslots,
                       max_msgs, (u64)src_len, L.ntiles, agg, d_send_res, bo64, loc, (u64)tx_capacity, lead, flags, rec, ptr, tx_off,
                       reinterpret_cast<u64*>(d_msg_tx_off));
    if (tx_capacity)
        hipLaunchKernelGGL(ws_send_emit, dim3((u32)L.npieces), dim3(SEND_T), 0, st, d_src, (u64)src_len, nseg, nslots, rec, ptr, tx_off, d_tx,
                           (u64)tx_capacity, lead);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (snprintf(text, sizeof text, "%s launch", who), ws_set_err(text, e));
}

extern "C" WSFRAME_AMD_SEND_EXPORT int websocketframeBatchSendDevice(
    const unsigned char* d_src, unsigned long long src_len, const WebsocketSendMsg_t* d_msg, const unsigned int* d_nmsg,
    unsigned int nseg, unsigned int max_msgs, const unsigned int* d_frag_size, const unsigned int* d_mask_key,
    unsigned int flags, unsigned char* d_tx, unsigned long long tx_capacity, unsigned long long* d_tx_off,
    unsigned long long* d_msg_tx_off, WebsocketSendResult_t* d_send_res, void* hip_stream) {
    if (flags) return ws_set_msg("websocketframeBatchSendDevice: unknown flag");
    return send_batch("websocketframeBatchSendDevice", d_src, src_len, d_msg, d_nmsg, nseg, max_msgs, d_frag_size, d_mask_key, 0u, d_tx,
                      tx_capacity, d_tx_off, d_msg_tx_off, d_send_res, hip_stream);
}

extern "C" WSFRAME_AMD_PMD_EXPORT int websocketframeBatchSendExtDevice(
    const unsigned char* d_src, unsigned long long src_len, const WebsocketSendMsg_t* d_msg, const unsigned int* d_nmsg,
    unsigned int nseg, unsigned int max_msgs, const unsigned int* d_frag_size, const unsigned int* d_mask_key,
    unsigned int flags, unsigned char* d_tx, unsigned long long tx_capacity, unsigned long long* d_tx_off,
    unsigned long long* d_msg_tx_off, WebsocketSendResult_t* d_send_res, void* hip_stream) {
    if (flags & ~WEBSOCKET_SEND_FLAG_RSV1) return ws_set_msg("websocketframeBatchSendExtDevice: unknown flag");
    return send_batch("websocketframeBatchSendExtDevice", d_src, src_len, d_msg, d_nmsg, nseg, max_msgs, d_frag_size, d_mask_key, flags,
                      d_tx, tx_capacity, d_tx_off, d_msg_tx_off, d_send_res, hip_stream);
}

extern "C" WSFRAME_AMD_SEND_EXPORT int websocketframeBatchSendListFromMessagesDevice(
    const WebsocketFrameDesc_t* d_desc, const WebsocketMsgDesc_t* d_msg, const unsigned int* d_nmsg, unsigned int nseg,
    unsigned int max_frames, WebsocketSendMsg_t* d_send_msg, void* hip_stream) {
    if (max_frames == 0) return ws_set_msg("websocketframeBatchSendListFromMessagesDevice: invalid argument (max_frames 0)");
    if (nseg && (!d_desc || !d_msg || !d_nmsg || !d_send_msg))
        return ws_set_msg("websocketframeBatchSendListFromMessagesDevice: invalid argument (NULL pointer)");
    if ((reinterpret_cast<uintptr_t>(d_desc) | reinterpret_cast<uintptr_t>(d_msg)) & 15)
        return ws_set_msg("websocketframeBatchSendListFromMessagesDevice: d_desc/d_msg not 16-B aligned");
    if ((reinterpret_cast<uintptr_t>(d_send_msg) & 7) || (reinterpret_cast<uintptr_t>(d_nmsg) & 3))
        return ws_set_msg("websocketframeBatchSendListFromMessagesDevice: d_send_msg not 8-B or d_nmsg not 4-B aligned");
    const u64 nslots = (u64)nseg * max_frames;
    if (nslots > (1ull << 30)) return ws_set_msg("websocketframeBatchSendListFromMessagesDevice: nseg * max_frames > 2^30");
    if (nslots == 0) return 0;
    hipLaunchKernelGGL(ws_send_list, dim3((u32)((nslots + SEND_T - 1) / SEND_T)), dim3(SEND_T), 0,
                       reinterpret_cast<hipStream_t>(hip_stream), d_desc, d_msg, d_nmsg, (u32)nslots, max_frames, d_send_msg);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchSendListFromMessagesDevice launch", e);
}

extern "C" WSFRAME_AMD_SEND_EXPORT long long websocketframeSendHost(
    const unsigned char* src, unsigned long long src_len, const WebsocketSendMsg_t* msg, unsigned int nmsg,
    unsigned int frag_size, const unsigned int* mask_key, unsigned int flags, unsigned char* tx,
    unsigned long long tx_capacity, unsigned long long* msg_tx_off, WebsocketSendResult_t* out) {
    if (flags) return ws_set_msg("websocketframeSendHost: unknown flag");
    if (!src || !out || (!msg && nmsg) || (!tx && tx_capacity))
        return ws_set_msg("websocketframeSendHost: invalid argument (NULL pointer)");
    if (src_len > WS_SEND_SRC_MAX) return ws_set_msg("websocketframeSendHost: src_len > 2^56");
    return (long long)ws_send_connection(src, src_len, msg, nmsg, frag_size, mask_key, tx, tx_capacity,
                                         reinterpret_cast<uint64_t*>(msg_tx_off), out);
}

extern "C" WSFRAME_AMD_PMD_EXPORT long long websocketframeSendExtHost(
    const unsigned char* src, unsigned long long src_len, const WebsocketSendMsg_t* msg, unsigned int nmsg,
    unsigned int frag_size, const unsigned int* mask_key, unsigned int flags, unsigned char* tx,
    unsigned long long tx_capacity, unsigned long long* msg_tx_off, WebsocketSendResult_t* out) {
    if (flags & ~WEBSOCKET_SEND_FLAG_RSV1) return ws_set_msg("websocketframeSendExtHost: unknown flag");
    if (!src || !out || (!msg && nmsg) || (!tx && tx_capacity))
        return ws_set_msg("websocketframeSendExtHost: invalid argument (NULL pointer)");
    if (src_len > WS_SEND_SRC_MAX) return ws_set_msg("websocketframeSendExtHost: src_len > 2^56");
    return (long long)ws_send_connection_ext(src, src_len, msg, nmsg, frag_size, mask_key, flags, tx, tx_capacity,
                                             reinterpret_cast<uint64_t*>(msg_tx_off), out);
}
