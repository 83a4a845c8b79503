// A thin C shim over util_amd/csrc/ws_rwplan.h (the chunk, window and part geometry of the raw
// stream's chunk-parallel walk) for tests/test_rwplan_host.py, which holds it against the independent
// model in tests/rwplan_model.py.
#include "../../util_amd/csrc/ws_rwplan.h"

// in[13] = P1, len, mean, longest, cmin, cmax, nchunks_cap, cand_cap, stg_cap, split_x0, split_x1,
// shift0, shift1. out[2 + 9 k ..] = nparts, nchunks, then per part P, C, H, n, cbase, capc, stgn,
// stg_base, cand_base. Returns 0, or -1 for inputs outside what the library ever passes (an empty
// rest, caps below RW_NP chunks of the smallest lists: no chunk size would fit them).
extern "C" int ws_rwplan_device(const uint64_t* in, uint64_t* out) {
    RwPlanIn I;
    I.P1 = in[0]; I.len = in[1]; I.mean = in[2]; I.longest = (u32)in[3]; I.cmin = in[4]; I.cmax = in[5];
    I.nchunks_cap = (u32)in[6]; I.cand_cap = in[7]; I.stg_cap = in[8];
    I.split_x[0] = in[9]; I.split_x[1] = in[10]; I.shift[0] = (u32)in[11]; I.shift[1] = (u32)in[12];
    if (I.P1 >= I.len || I.len >> 48 || I.nchunks_cap < RW_NP || I.cand_cap < RW_NP * 64 || I.stg_cap < RW_NP * RW_D * 64 ||
        I.shift[0] > 6 || I.shift[1] > 6 || I.cmin < RW_CMIN || (I.cmin & (I.cmin - 1)) || (I.cmax & (I.cmax - 1)))
        return -1;
    const RwGeom G = rw_plan_geometry(I);
    out[0] = G.nparts;
    out[1] = G.nchunks;
    for (int k = 0; k < RW_NP; ++k) {
        const RwPart& t = G.pt[k];
        uint64_t* o = out + 2 + 9 * k;
        o[0] = t.P; o[1] = t.C; o[2] = t.H; o[3] = t.n; o[4] = t.cbase; o[5] = t.capc; o[6] = t.stgn;
        o[7] = t.stg_base; o[8] = t.cand_base;
    }
    return 0;
}

// out[5] = C, H, nchunks, stgn, capc of the host-linked walk
extern "C" void ws_rwplan_hostgeo(uint64_t P1, uint64_t len, uint64_t mean, uint64_t cmax, uint64_t* out) {
    const RwHostGeom G = rw_host_geometry(P1, len, mean, cmax);
    out[0] = G.C; out[1] = G.H; out[2] = G.nchunks; out[3] = G.stgn; out[4] = G.capc;
}

extern "C" uint32_t ws_rwplan_window(uint64_t mean, uint32_t maxlen, uint64_t C) { return rw_window(mean, maxlen, C); }
extern "C" uint64_t ws_rwplan_mean(uint64_t P, uint64_t P1, uint64_t frames) { return rw_sample_mean(P, P1, frames); }
extern "C" int ws_rwplan_short_rest(uint64_t P1, uint64_t len, uint64_t mean) { return rw_short_rest(P1, len, mean) ? 1 : 0; }
// out[] = the constants a model needs to be told (it states the others itself)
extern "C" void ws_rwplan_consts(uint64_t* out) {
    out[0] = RW_CMIN; out[1] = RW_CMAX; out[2] = RW_HMIN; out[3] = RW_HMAX; out[4] = RW_SAMPLE; out[5] = RW_MIN;
    out[6] = RW_MIN_FRAMES; out[7] = RW_NP; out[8] = RW_D; out[9] = RW_CAP_STGN; out[10] = RW_STG; out[11] = RW_CAP_CHUNKS;
}

#ifdef WS_RWPLAN_MAIN
// a stand-alone run over directed and random inputs (for a sanitizer build of the header: -DWS_RWPLAN_MAIN)
#include <cstdio>
int main() {
    uint64_t x = 88172645463325252ull, sum = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const uint64_t means[] = {0, 1, 63, 64, 65, 4096, 70000, 1 << 20};
    const uint64_t seens[] = {0, 1, 4095, 4096, (128 << 10) - 4096, (128 << 10) - 4095, 0xFFFFFFFFull};
    for (int it = 0; it < 200000; ++it) {
        uint64_t in[13], out[2 + 9 * RW_NP], h[5];
        in[0] = rnd() % (1 << 20);
        in[1] = in[0] + 1 + (it % 3 ? rnd() % (64 << 20) : (rnd() % 40) * 65536 + rnd() % 3);
        in[2] = means[rnd() % 8] + (it % 7 == 0 ? rnd() % 5000 : 0);
        in[3] = seens[rnd() % 7];
        in[4] = RW_CMIN << (rnd() % 4);
        in[5] = 1ull << (16 + rnd() % 11);
        in[6] = 3 + rnd() % (it % 2 ? 40 : 40000);
        in[7] = 192 + rnd() % (it % 2 ? 5000 : 5000000);
        in[8] = 768 + rnd() % (it % 2 ? 20000 : 20000000);
        in[9] = it % 5 ? rnd() % (in[1] + 70000) : 0;
        in[10] = it % 4 ? rnd() % (in[1] + 70000) : 0;
        in[11] = rnd() % 7;
        in[12] = rnd() % 7;
        if (ws_rwplan_device(in, out) == 0)
            for (int i = 0; i < 2 + 9 * RW_NP; ++i) sum += out[i];
        ws_rwplan_hostgeo(in[0], in[1], in[2], in[5], h);
        sum += h[0] + h[1] + h[2] + h[3] + h[4] + ws_rwplan_window(in[2], (uint32_t)in[3], in[5]) +
               ws_rwplan_mean(0, in[0], it % 9) + ws_rwplan_short_rest(in[0], in[1], in[2]);
    }
    printf("ok %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
