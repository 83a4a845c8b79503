// ws_hostplan.h — the host-side plan of websocketframeBatchDecodeHost(Multi), ws_hostpath.hip:
// which segments form a group (one H2D copy, one decode, one slot), which host ranges a group
// writes back, and where a multi-device call cuts the segments. Plain C++17, no HIP: the one
// definition the library runs and tests/c/hostplan_host.cpp holds against an independent model
// (tests/test_hostplan_host.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#define WS_HOSTPLAN_DESC_BYTES 32ull              // sizeof(WebsocketFrameDesc_t)
#define WS_HOSTPLAN_DESC_CAP (64ull << 20)        // descriptor bytes of one group (its D2H copy and device slot)

// (the segment arrays are a template parameter U: any unsigned 64-bit type, the C ABI's unsigned long long
// or uint64_t)
struct WsHostGroup {
    uint32_t s0, s1;   // segments [s0, s1)
    uint64_t lo, hi;   // host byte span [lo, hi): the min offset and the max end of its segments
};

struct WsHostPlan {
    bool outside = false;             // a segment does not lie in [0, buflen]: nothing else is set
    bool ordered = true;              // every segment starts at or after the end of the one before it
    std::vector<WsHostGroup> groups;  // in segment order; they partition [0, nseg)
    uint64_t max_span = 0;            // the largest hi - lo
    uint32_t max_nseg = 0;            // the largest s1 - s0 (the two may come from different groups)
};

// every segment lies in [0, buflen] (an empty one may sit at buflen)
template <typename U>
inline bool ws_host_inside(const U* seg_off, const U* seg_len, uint32_t nseg, uint64_t buflen) {
    static_assert(sizeof(U) == 8 && U(-1) > U(0), "64-bit unsigned offsets");
    for (uint32_t s = 0; s < nseg; ++s)
        if (seg_off[s] > buflen || seg_len[s] > buflen - seg_off[s]) return false;
    return true;
}

// ascending and non-overlapping, in the order given (zero-length segments may touch anything)
template <typename U>
inline bool ws_host_ordered(const U* seg_off, const U* seg_len, uint32_t nseg) {
    uint64_t prev_end = 0;
    for (uint32_t s = 0; s < nseg; ++s) {
        if (seg_off[s] < prev_end) return false;
        prev_end = seg_off[s] + seg_len[s];
    }
    return true;
}

// Groups of consecutive segments. Ordered segments: a group takes the next segment while its span
// from the group's first offset to that segment's end is at most chunk_bytes and the descriptors of
// its segments (max_frames each) are at most desc_cap_bytes; a group always holds its first segment,
// whatever its size. Any other layout is one group spanning all segments.
template <typename U>
inline WsHostPlan ws_host_plan(const U* seg_off, const U* seg_len, uint32_t nseg, uint32_t max_frames,
                               uint64_t buflen, uint64_t chunk_bytes, uint64_t desc_cap_bytes = WS_HOSTPLAN_DESC_CAP) {
    WsHostPlan P;
    if (!ws_host_inside(seg_off, seg_len, nseg, buflen)) {
        P.outside = true;
        return P;
    }
    uint64_t lo_all = ~0ull, hi_all = 0;
    for (uint32_t s = 0; s < nseg; ++s) {
        const uint64_t o = seg_off[s], l = seg_len[s];
        lo_all = o < lo_all ? o : lo_all;
        hi_all = o + l > hi_all ? o + l : hi_all;
    }
    P.ordered = ws_host_ordered(seg_off, seg_len, nseg);
    if (nseg == 0) return P;
    if (!P.ordered) {
        P.groups.push_back(WsHostGroup{0, nseg, lo_all, hi_all});
    } else {
        // segments whose descriptors fit the cap: n * max_frames * 32 <= cap, without the product
        const uint64_t per_seg = (uint64_t)max_frames * WS_HOSTPLAN_DESC_BYTES;
        const uint64_t cap_segs = per_seg ? desc_cap_bytes / per_seg : ~0ull;
        for (uint32_t s = 0; s < nseg;) {
            WsHostGroup g{s, s + 1, seg_off[s], (uint64_t)(seg_off[s] + seg_len[s])};
            while (g.s1 < nseg) {
                const uint64_t end = seg_off[g.s1] + seg_len[g.s1];
                if (end - g.lo > chunk_bytes) break;
                if ((uint64_t)(g.s1 + 1 - g.s0) > cap_segs) break;
                g.hi = end;
                ++g.s1;
            }
            P.groups.push_back(g);
            s = g.s1;
        }
    }
    for (const WsHostGroup& g : P.groups) {
        P.max_span = g.hi - g.lo > P.max_span ? g.hi - g.lo : P.max_span;
        P.max_nseg = g.s1 - g.s0 > P.max_nseg ? g.s1 - g.s0 : P.max_nseg;
    }
    return P;
}

// The host ranges [first, second) a group writes back: the bytes of its non-empty segments in
// buffer order, ranges that touch or overlap merged into one. Bytes between segments are in no range.
template <typename U>
inline void ws_host_back_ranges(const U* seg_off, const U* seg_len, const WsHostGroup& g, bool ordered,
                                std::vector<std::pair<uint64_t, uint64_t>>& out) {
    std::vector<std::pair<uint64_t, uint64_t>> r;
    r.reserve(g.s1 - g.s0);
    for (uint32_t s = g.s0; s < g.s1; ++s)
        if (seg_len[s]) r.emplace_back((uint64_t)seg_off[s], (uint64_t)(seg_off[s] + seg_len[s]));
    if (!ordered) std::sort(r.begin(), r.end());
    out.clear();
    for (const auto& x : r) {
        if (!out.empty() && x.first <= out.back().second)
            out.back().second = std::max(out.back().second, x.second);
        else
            out.push_back(x);
    }
}

// a multi-device call that runs as the one-device call on devices[0]
inline bool ws_host_multi_single(bool ordered, uint32_t nseg, int ndev) { return !ordered || ndev == 1 || nseg < 2; }

// Cuts of ordered segments into nd = min(ndev, nseg) contiguous ranges [cut[r], cut[r + 1]) of about
// equal bytes: cut[r] is the segment boundary nearest to the share total * r / nd, the lower boundary
// on a tie, and never below cut[r - 1] (a range may be empty). Empty segments put several boundaries
// at one byte position: at or below the share the last of them is the boundary, above it the first.
// total == 0 leaves every segment in range 0. ndev >= 1.
template <typename U>
inline std::vector<uint32_t> ws_host_cuts(const U* seg_len, uint32_t nseg, int ndev) {
    const uint32_t nd = (uint32_t)std::min<uint64_t>((uint64_t)ndev, nseg);
    std::vector<uint32_t> cut(nd + 1, 0);
    cut[nd] = nseg;
    uint64_t total = 0;
    for (uint32_t s = 0; s < nseg; ++s) total += seg_len[s];
    uint64_t acc = 0;
    uint32_t s = 0;
    for (uint32_t r = 1; r < nd; ++r) {
        const long double t = (long double)total * r / nd;
        while (s < nseg && (long double)(acc + seg_len[s]) <= t) acc += seg_len[s++];
        // acc <= t < acc + len[s]: the nearer boundary
        if (s < nseg && (long double)(acc + seg_len[s]) - t < t - (long double)acc) acc += seg_len[s++];
        cut[r] = std::max(s, cut[r - 1]);
    }
    return cut;
}
