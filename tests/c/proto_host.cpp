// Host driver of util_amd/csrc/ws_proto.h (tests/test_proto_host.py): the header's one-frame step
// for sweeps against the oracle, and the header's summary combine folded over every cut of a
// frame sequence into tiles, held against that step. Built as a shared library for ctypes and,
// with -DPROTO_HOST_MAIN, as a program of its own (the fold checks; the build for sanitizers).
#include <stdint.h>
#include <stdio.h>

#include "../../util_amd/csrc/ws_proto.h"

extern "C" {

// n independent frames: frame i arrives on a connection in state st_in[i]
void ws_proto_host_steps(uint32_t n, const uint64_t* st_in, const uint8_t* b0, const uint8_t* masked,
                         const uint64_t* datalen, const uint16_t* close_code, uint32_t flags, uint32_t rsv_allowed,
                         uint64_t limit, uint8_t* code_out, uint64_t* st_out) {
    const WsProtoCfg cfg{flags, rsv_allowed, limit};
    for (uint32_t i = 0; i < n; ++i) {
        WsProtoFrame f;
        f.b0 = b0[i]; f.type = b0[i] & 15u; f.fin = b0[i] >> 7; f.masked = masked[i]; f.datalen = datalen[i];
        f.close_code = close_code[i];
        uint64_t st = st_in[i];
        code_out[i] = (uint8_t)ws_proto_step(&st, f, cfg);
        st_out[i] = st;
    }
}

// The frame alphabet of the fold checks: what moves the state in every way it can move.
static const WsProtoFrame ALPHABET[6] = {
    {0x01, 1, 0, 1, 0, 2},      // TEXT, no FIN, 2 bytes
    {0x00, 0, 0, 1, 0, 1},      // CONT, no FIN, 1 byte
    {0x80, 0, 1, 1, 0, 3},      // CONT, FIN, 3 bytes
    {0x82, 2, 1, 1, 0, 1},      // BINARY, FIN, 1 byte
    {0x89, 9, 1, 1, 0, 0},      // PING
    {0x88, 8, 1, 1, 1000, 2},   // CLOSE 1000
};

// One sequence of n <= 12 symbols from state st: the sequential step against the fold over
// every cut into tiles (2^(n-1) cuts). Returns the number of cuts that disagree anywhere.
static uint32_t fold_check(const uint8_t* sym, uint32_t n, uint64_t st, const WsProtoCfg& cfg) {
    uint8_t want[12];
    uint64_t run = st;
    for (uint32_t k = 0; k < n; ++k) want[k] = (uint8_t)ws_proto_step(&run, ALPHABET[sym[k]], cfg);
    const uint32_t closed = (uint32_t)((st & WS_PROTO_ST_CLOSED) != 0);
    uint32_t bad = 0;
    for (uint32_t cuts = 0; cuts < (n ? 1u << (n - 1) : 1u); ++cuts) {     // bit k: a tile ends after frame k
        WsProtoSum tile[12];
        uint32_t first[13], nt = 0;
        first[0] = 0;
        for (uint32_t k = 0; k < n; ++k) {
            const WsProtoFrame& f = ALPHABET[sym[k]];
            const WsProtoSum s = ws_proto_sum_frame(f.type, f.fin, f.datalen, k);
            tile[nt] = k == first[nt] ? s : ws_proto_comb(tile[nt], s);
            if (k == n - 1 || (cuts >> k) & 1u) first[++nt] = k + 1;
        }
        bool ok = true;
        WsProtoSum carry = ws_proto_sum_none();
        for (uint32_t t = 0; t < nt; ++t) {
            WsProtoSum in = ws_proto_sum_none();
            for (uint32_t k = first[t]; k < first[t + 1]; ++k) {
                const WsProtoFrame& f = ALPHABET[sym[k]];
                const WsProtoSum before = ws_proto_comb(ws_proto_sum_state(st), ws_proto_comb(carry, in));
                ok &= ws_proto_code(before, closed, f, cfg) == want[k];
                in = ws_proto_comb(in, ws_proto_sum_frame(f.type, f.fin, f.datalen, k));
            }
            carry = ws_proto_comb(carry, tile[t]);
        }
        ok &= ws_proto_state_out(st, carry) == run;
        bad += !ok;
    }
    return bad;
}

static const uint64_t STATES[4] = {0, WS_PROTO_ST_OPEN | 2, WS_PROTO_ST_OPEN | 4, WS_PROTO_ST_CLOSED};

// every sequence of 0..maxlen symbols, from each state, with limit 4
uint64_t ws_proto_host_fold_all(uint32_t maxlen) {
    const WsProtoCfg cfg{WS_PROTO_F_EXPECT_MASKED, 0, 4};
    uint64_t bad = 0;
    for (uint32_t n = 0; n <= maxlen && n <= 12; ++n) {
        uint64_t total = 1;
        for (uint32_t i = 0; i < n; ++i) total *= 6;
        for (uint64_t v = 0; v < total; ++v) {
            uint8_t sym[12];
            uint64_t r = v;
            for (uint32_t i = 0; i < n; ++i) { sym[i] = (uint8_t)(r % 6); r /= 6; }
            for (uint64_t st : STATES) bad += fold_check(sym, n, st, cfg);
        }
    }
    return bad;
}

// `count` seeded random sequences of n symbols (CLOSE one time in 24, so that most run long)
uint64_t ws_proto_host_fold_random(uint64_t seed, uint32_t count, uint32_t n) {
    const WsProtoCfg cfg{0, 0, 5};
    uint64_t bad = 0, x = seed * 0x9E3779B97F4A7C15ull + 1;
    for (uint32_t c = 0; c < count; ++c) {
        uint8_t sym[12];
        for (uint32_t i = 0; i < n && i < 12; ++i) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;                    // xorshift64
            const uint32_t r = (uint32_t)(x >> 33) % 120;
            sym[i] = r < 5 ? 5 : (uint8_t)(r % 5);
        }
        bad += fold_check(sym, n < 12 ? n : 12, STATES[c & 3], cfg);
    }
    return bad;
}

}  // extern "C"

#ifdef PROTO_HOST_MAIN
int main() {
    // (a tenth of what tests/test_proto_host.py folds through the shared library: this build is the one for sanitizers)
    const uint64_t a = ws_proto_host_fold_all(5), b = ws_proto_host_fold_random(6455, 1000, 12);
    if (a || b) {
        printf("proto_host: %llu + %llu cuts disagree with the sequential step\n", (unsigned long long)a, (unsigned long long)b);
        return 1;
    }
    printf("proto_host ok\n");
    return 0;
}
#endif
