// ws_scan.h — the launch skeleton of the entry points that plan on the device (ws_utf8.hip,
// ws_proto.hip, ws_reply.hip, ws_send.hip), written once:
//   plan     a per-block exclusive sum of counts (ws_block_sum), then one block's exclusive scan of
//            the block sums (ws_offsets_scan);
//   tiles    a fixed grid over tiles of 256 list items, one per thread: a wave finds the segments of
//            its first and last item by a 64-ary search (ws_wave_search) over the list starts, a lane
//            its own between the two (ws_list_locate; ws_frame_mine for a list of frames); the
//            block's segmented scan of the items' summaries (ws_seg_block_scan) leaves the tile's;
//   combine  one block's exclusive segmented scan of the tile summaries (ws_seg_combine);
//   again    the tiles once more, now with the tile's carry in front of each item (ws_seg_before),
//            or per segment: its last tile's part behind that tile's carry (ws_seg_fold).
// A summary is described by an ops struct: its type Sum (a `bits` word with the HEAD flag: the run
// starts a new segment), none(), comb() and comb_seg(); the three in use wrap ws_proto.h's,
// ws_reply.h's and ws_send.h's host-tested functions. Records travel as whole words (ws_ld, ws_st,
// ws_shfl_up, ws_shfl): their layout is stated once, by their struct.
// Device side only; the __global__ kernels stay in the .hip files, thin wrappers where a kernel is
// one of these bodies.
#pragma once
#include <type_traits>

#include "ws_common.h"

// ---------------------------------------------------------------------------------------------
// Word-wise record I/O: any trivially copyable record of whole 16-B units (4-B words for the
// shuffles), as u32x4 global loads / stores and one shuffle per word. Pad fields travel as they
// are: whoever builds a record sets them (to 0).
template <typename R>
struct WsWords {
    u32 w[sizeof(R) / 4];
};

template <typename R>
__device__ __forceinline__ R ws_ld(const R* p) {
    static_assert(std::is_trivially_copyable<R>::value && sizeof(R) % 16 == 0, "a record of whole 16-B units");
    const gu32x4* const g = gptr<u32x4>(p);
    WsWords<R> w;
#pragma unroll
    for (u32 i = 0; i < sizeof(R) / 16; ++i) {
        const u32x4 v = g[i];
        w.w[4 * i] = v.x; w.w[4 * i + 1] = v.y; w.w[4 * i + 2] = v.z; w.w[4 * i + 3] = v.w;
    }
    return __builtin_bit_cast(R, w);
}

template <typename R>
__device__ __forceinline__ void ws_st(R* p, const R& r) {
    static_assert(std::is_trivially_copyable<R>::value && sizeof(R) % 16 == 0, "a record of whole 16-B units");
    const WsWords<R> w = __builtin_bit_cast(WsWords<R>, r);
    gu32x4* const g = gptr<u32x4>(p);
#pragma unroll
    for (u32 i = 0; i < sizeof(R) / 16; ++i) {
        u32x4 v;
        v.x = w.w[4 * i]; v.y = w.w[4 * i + 1]; v.z = w.w[4 * i + 2]; v.w = w.w[4 * i + 3];
        g[i] = v;
    }
}

template <typename R>
__device__ __forceinline__ R ws_shfl_up(const R& r, int d) {
    static_assert(std::is_trivially_copyable<R>::value && sizeof(R) % 4 == 0, "a record of whole words");
    WsWords<R> w = __builtin_bit_cast(WsWords<R>, r);
#pragma unroll
    for (u32 i = 0; i < sizeof(R) / 4; ++i) w.w[i] = (u32)__shfl_up((int)w.w[i], d);
    return __builtin_bit_cast(R, w);
}

template <typename R>
__device__ __forceinline__ R ws_shfl(const R& r, int src) {
    static_assert(std::is_trivially_copyable<R>::value && sizeof(R) % 4 == 0, "a record of whole words");
    WsWords<R> w = __builtin_bit_cast(WsWords<R>, r);
#pragma unroll
    for (u32 i = 0; i < sizeof(R) / 4; ++i) w.w[i] = (u32)__shfl((int)w.w[i], src);
    return __builtin_bit_cast(R, w);
}

// ---------------------------------------------------------------------------------------------
// plan

// Exclusive sum of v (u32 or u64) over the block's NT threads in thread order into *excl; the
// block's sum is returned. wsum: NT / 64 values of LDS, used by one call per kernel.
template <u32 NT, typename T>
__device__ __forceinline__ T ws_block_sum(T v, T* wsum, T* excl) {
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = ws_shfl_up(inc, d);
        if (lane >= (u32)d) inc += o;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    T base = 0, total = 0;
#pragma unroll
    for (u32 k = 0; k < NT / 64; ++k) {
        if (k < wv) base += wsum[k];
        total += wsum[k];
    }
    *excl = base + inc - v;
    return total;
}

// One block of 1024 threads: exclusive scan of the nb block sums in place; bo[nb] and *total_out
// take the total. part: 1024 values of LDS.
template <typename T>
__device__ __forceinline__ void ws_offsets_scan(T* bo, u32 nb, T* total_out, T* part) {
    const u32 t = threadIdx.x, per = (nb + 1023) / 1024;
    const u32 lo = t * per < nb ? t * per : nb, hi = lo + per < nb ? lo + per : nb;
    T sum = 0;
    for (u32 k = lo; k < hi; ++k) sum += bo[k];
    part[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < 1024; d <<= 1) {
        const T o = t >= d ? part[t - d] : (T)0;
        __syncthreads();
        part[t] += o;
        __syncthreads();
    }
    T run = part[t] - sum;
    for (u32 k = lo; k < hi; ++k) {
        const T v = bo[k];
        bo[k] = run;
        run += v;
    }
    if (t == 1023) {
        bo[nb] = part[1023];
        total_out[0] = part[1023];
    }
}

// ---------------------------------------------------------------------------------------------
// segmented scans

// Segmented scan (Ops::comb_seg) over the block's NT values in thread order: *excl takes the fold
// of the values before this thread, the fold of all of them is returned. wsum: NT / 64 summaries
// of LDS; a kernel may call this once per tile.
template <u32 NT, typename Ops>
__device__ __forceinline__ typename Ops::Sum ws_seg_block_scan(typename Ops::Sum v, typename Ops::Sum* wsum,
                                                               typename Ops::Sum* excl) {
    typedef typename Ops::Sum Sum;
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const Sum o = ws_shfl_up(v, d);
        if (lane >= (u32)d) v = Ops::comb_seg(o, v);
    }
    Sum e = ws_shfl_up(v, 1);
    if (lane == 0) e = Ops::none();
    __syncthreads();                                   // (the previous tile's readers of wsum are done)
    if (lane == 63) wsum[wv] = v;
    __syncthreads();
    Sum base = Ops::none(), total = Ops::none();
#pragma unroll
    for (u32 k = 0; k < NT / 64; ++k) {
        const Sum w = wsum[k];
        if (k < wv) base = Ops::comb_seg(base, w);
        total = Ops::comb_seg(total, w);
    }
    *excl = Ops::comb_seg(base, e);
    return total;
}

// One block of 1024 threads: exclusive segmented scan of the nt tile summaries in place (agg[t]:
// what tile t's first segment brings along from the tiles before). part: 1024 summaries of LDS.
template <typename Ops>
__device__ __forceinline__ void ws_seg_combine(typename Ops::Sum* agg, u32 nt, typename Ops::Sum* part) {
    typedef typename Ops::Sum Sum;
    const u32 t = threadIdx.x, per = (nt + 1023) / 1024;
    const u32 lo = t * per < nt ? t * per : nt, hi = lo + per < nt ? lo + per : nt;
    Sum sum = Ops::none();
    for (u32 k = lo; k < hi; ++k) sum = Ops::comb_seg(sum, ws_ld(agg + k));
    part[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < 1024; d <<= 1) {
        const Sum o = t >= d ? part[t - d] : Ops::none();
        __syncthreads();
        part[t] = Ops::comb_seg(o, part[t]);
        __syncthreads();
    }
    Sum run = t ? part[t - 1] : Ops::none();
    for (u32 k = lo; k < hi; ++k) {
        const Sum v = ws_ld(agg + k);
        ws_st(agg + k, run);
        run = Ops::comb_seg(run, v);
    }
}

// The items of this item's segment before it, from ws_seg_block_scan's *excl: none (the segment's
// first item), those of this tile (the segment starts in it: HEAD), or those with the tiles
// before (carry: this tile's entry of the combined agg).
template <typename Ops>
__device__ __forceinline__ typename Ops::Sum ws_seg_before(const typename Ops::Sum& excl, bool first,
                                                           const typename Ops::Sum* carry) {
    if (first) return Ops::none();
    if (excl.bits & Ops::HEAD) return excl;
    return Ops::comb(ws_ld(carry), excl);
}

// The fold of all n > 0 items of the segment whose first item stands at list position `start`:
// its items inside its last tile (*tail: stored by that tile for the segment's last item), behind
// those of the tiles before where it does not start in that tile.
template <u32 NT, typename Ops>
__device__ __forceinline__ typename Ops::Sum ws_seg_fold(const typename Ops::Sum* tail, const typename Ops::Sum* agg,
                                                         u64 start, u64 n) {
    const u64 tl = (start + n - 1) / NT;
    const typename Ops::Sum all = ws_ld(tail);
    return start < tl * NT ? Ops::comb(ws_ld(agg + tl), all) : all;
}

// ---------------------------------------------------------------------------------------------
// the list

// The largest i in [0, n) with start(i) <= f (start non-decreasing, start(0) <= f, f wave-uniform),
// by the whole wave: 64 probes a round.
template <typename F>
__device__ __forceinline__ u32 ws_wave_search(F start, u32 n, u32 f, u32 lane) {
    u32 lo = 0, hi = n;
    while (hi - lo > 1) {
        const u32 step = (hi - lo + 63) / 64;
        const u64 idx = (u64)lo + (u64)lane * step;
        const bool le = idx < hi && start((u32)idx) <= f;
        const u32 cnt = (u32)__popcll(__ballot(le));   // >= 1: lane 0 probes lo
        lo += (cnt - 1) * step;
        hi = hi < lo + step ? hi : lo + step;
    }
    return lo;
}

// The list of the counted frames of all segments, laid end to end in segment order: bo[b] is the
// list position of plan block b's first segment, loff[s] segment s's inside its block of NT.
template <u32 NT>
__device__ __forceinline__ u32 ws_list_start(const u32* bo, const u32* loff, u32 s) {
    return bo[s / NT] + loff[s];
}

// This thread's item of tile t, list position t * NT + threadIdx.x: false past the `total` items;
// else its segment *s (the last one that starts at or before it: not an empty one) and its index
// *k in it. Whole waves call this (total <= 2^30: no wrap).
template <u32 NT>
__device__ __forceinline__ bool ws_list_locate(u32 t, u32 total, const u32* bo, const u32* loff, u32 nseg, u32* s, u32* k) {
    const u32 lane = threadIdx.x & 63;
    const u32 f0 = t * NT + (threadIdx.x & ~63u), f = f0 + lane;
    if (f0 >= total) return false;                     // (wave-uniform)
    const auto start = [&](u32 i) { return ws_list_start<NT>(bo, loff, i); };
    const u32 f1 = f0 + 63 < total ? f0 + 63 : total - 1;
    const u32 s0 = ws_wave_search(start, nseg, f0, lane);
    const u32 s1 = f1 == f0 ? s0 : ws_wave_search(start, nseg, f1, lane);
    if (f >= total) return false;
    u32 lo = s0, hi = s1 + 1;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (start(mid) <= f) lo = mid;
        else hi = mid;
    }
    *s = lo;
    *k = f - start(lo);
    return true;
}

// a segment's counted frames (n_frames, at most max_frames); *consumed takes its consumed bytes
__device__ __forceinline__ u32 ws_seg_count(const WebsocketSegResult_t* res, u32 s, u32 max_frames, u64* consumed) {
    const u32x4 r = *gptr<u32x4>(res + s);
    *consumed = (u64)r.x | (u64)r.y << 32;
    return r.z < max_frames ? r.z : max_frames;
}

// a 32-B frame descriptor, by two 16-B loads
struct WsDesc {
    u64 frame_off, data_off, datalen;
    int ret;
    u32 fin, type, masked;
};
__device__ __forceinline__ WsDesc ws_desc_ld(const WebsocketFrameDesc_t* p) {
    const gu32x4* const g = gptr<u32x4>(p);
    const u32x4 d0 = g[0], d1 = g[1];
    WsDesc d;
    d.frame_off = (u64)d0.x | (u64)d0.y << 32;
    d.data_off = (u64)d0.z | (u64)d0.w << 32;
    d.datalen = (u64)d1.x | (u64)d1.y << 32;
    d.ret = (int)d1.z;
    d.fin = d1.w & 0xFFu;
    d.type = (d1.w >> 8) & 0xFFu;
    d.masked = (d1.w >> 16) & 0xFFu;
    return d;
}

// This thread's frame of tile t: whether there is one, its segment s, its index k of the segment's
// n counted frames, its descriptor, and whether the decode call consumed it (a counted frame that
// stopped its segment is not: it ends past the segment's consumed bytes, or its ret is <= 0).
struct WsFrameMine {
    bool valid, consumed;
    u32 s, k, n;
    WsDesc d;
};
template <u32 NT>
__device__ __forceinline__ WsFrameMine ws_frame_mine(u32 t, u32 total, const u32* bo, const u32* loff, u32 nseg, u32 max_frames,
                                                     const u64* seg_off, const WebsocketFrameDesc_t* desc,
                                                     const WebsocketSegResult_t* res) {
    WsFrameMine m = {};
    m.valid = ws_list_locate<NT>(t, total, bo, loff, nseg, &m.s, &m.k);
    if (!m.valid) return m;
    u64 consumed;
    m.n = ws_seg_count(res, m.s, max_frames, &consumed);
    m.d = ws_desc_ld(desc + ((u64)m.s * max_frames + m.k));
    m.consumed = m.d.ret > 0 && m.d.frame_off + (u64)m.d.ret <= seg_off[m.s] + consumed;
    return m;
}
