// A thin C shim over util_amd/csrc/ws_hostplan.h (the group plan, the write-back ranges and the
// multi-device cuts of the host-memory decode) for tests/test_hostplan_host.py, which holds it
// against the independent model in tests/host_cases.py.
#include "../../util_amd/csrc/ws_hostplan.h"

// groups[4 * g] = s0, s1, lo, hi. Returns the number of groups, -1 for a segment outside the buffer;
// *ordered, *max_span and *max_nseg as the plan has them. desc_cap_bytes 0: the header's default.
extern "C" long long ws_hostplan_groups(const uint64_t* seg_off, const uint64_t* seg_len, uint32_t nseg, uint32_t max_frames,
                                        uint64_t buflen, uint64_t chunk_bytes, uint64_t desc_cap_bytes, uint64_t* groups,
                                        int* ordered, uint64_t* max_span, uint32_t* max_nseg) {
    const WsHostPlan P = desc_cap_bytes ? ws_host_plan(seg_off, seg_len, nseg, max_frames, buflen, chunk_bytes, desc_cap_bytes)
                                        : ws_host_plan(seg_off, seg_len, nseg, max_frames, buflen, chunk_bytes);
    if (P.outside) return -1;
    *ordered = P.ordered ? 1 : 0;
    *max_span = P.max_span;
    *max_nseg = P.max_nseg;
    for (size_t g = 0; g < P.groups.size(); ++g) {
        groups[4 * g] = P.groups[g].s0;
        groups[4 * g + 1] = P.groups[g].s1;
        groups[4 * g + 2] = P.groups[g].lo;
        groups[4 * g + 3] = P.groups[g].hi;
    }
    return (long long)P.groups.size();
}

// ranges[2 * i] = first, one past the last; returns their number (at most s1 - s0)
extern "C" uint32_t ws_hostplan_ranges(const uint64_t* seg_off, const uint64_t* seg_len, uint32_t s0, uint32_t s1,
                                       uint64_t lo, uint64_t hi, int ordered, uint64_t* ranges) {
    std::vector<std::pair<uint64_t, uint64_t>> r;
    ws_host_back_ranges(seg_off, seg_len, WsHostGroup{s0, s1, lo, hi}, ordered != 0, r);
    for (size_t i = 0; i < r.size(); ++i) {
        ranges[2 * i] = r[i].first;
        ranges[2 * i + 1] = r[i].second;
    }
    return (uint32_t)r.size();
}

// cut[0 .. nd]; returns nd, or 0 when the call runs as the one-device call on devices[0]
extern "C" uint32_t ws_hostplan_cuts(const uint64_t* seg_off, const uint64_t* seg_len, uint32_t nseg, int ndev,
                                     uint32_t* cut) {
    if (ws_host_multi_single(ws_host_ordered(seg_off, seg_len, nseg), nseg, ndev)) return 0;
    const std::vector<uint32_t> c = ws_host_cuts(seg_len, nseg, ndev);
    for (size_t i = 0; i < c.size(); ++i) cut[i] = c[i];
    return (uint32_t)c.size() - 1;
}

#ifdef WS_HOSTPLAN_MAIN
// a stand-alone run over small layouts (for a sanitizer build of the header: -DWS_HOSTPLAN_MAIN)
#include <cstdio>
int main() {
    uint64_t x = 88172645463325252ull, sum = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int it = 0; it < 20000; ++it) {
        const uint32_t nseg = (uint32_t)(rnd() % 41);
        const uint64_t chunk = 1 + rnd() % 300, cap = 32 * (1 + rnd() % 6);
        std::vector<uint64_t> off(nseg + 1), len(nseg + 1);
        uint64_t at = rnd() % 7;
        for (uint32_t s = 0; s < nseg; ++s) {
            const uint64_t pick[6] = {0, 1, chunk - 1, chunk, chunk + 1, rnd() % 500};
            off[s] = at;
            len[s] = pick[rnd() % 6];
            at += len[s] + (rnd() % 3 ? 0 : rnd() % 400);
        }
        if (nseg > 2 && it % 5 == 0) std::swap(off[0], off[nseg - 1]), std::swap(len[0], len[nseg - 1]);
        std::vector<uint64_t> groups(4 * (nseg + 1)), ranges(2 * (nseg + 1));
        std::vector<uint32_t> cut(nseg + 2);
        int ordered = 0;
        uint64_t span = 0;
        uint32_t mn = 0;
        const long long ng = ws_hostplan_groups(off.data(), len.data(), nseg, 1 + it % 3, at - (it % 97 == 0), chunk, cap,
                                                groups.data(), &ordered, &span, &mn);
        for (long long g = 0; g < ng; ++g)
            sum += ws_hostplan_ranges(off.data(), len.data(), (uint32_t)groups[4 * g], (uint32_t)groups[4 * g + 1],
                                      groups[4 * g + 2], groups[4 * g + 3], ordered, ranges.data());
        sum += ws_hostplan_cuts(off.data(), len.data(), nseg, 1 + it % 9, cut.data()) + span + mn;
    }
    printf("ok %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
