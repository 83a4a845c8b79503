// One text message through the validator's own rule (util_amd/csrc/ws_utf8.h) compiled for the
// host: tests/test_text_host.py holds it against the oracle (tests/text_oracle.py).
#include <string.h>

#include "../../util_amd/csrc/ws_utf8.h"

// The bytes so far of a text message: the carry of `state_in` (continued != 0) followed by
// body[0, len). Returns 1 (valid) or 2 (invalid): a complete message must be well formed, an open
// one a prefix of a well-formed string. *state_out: the state word an open message leaves.
// phase < 0: one byte at a time (ws_utf8_byte_err). phase 0..15: as the kernel does, in 16-B
// chunks of a buffer in which the body starts at that phase, bytes outside the body masked to 0,
// the carried bytes placed before the first byte (ws_utf8_chunk_plain / ws_utf8_chunk_err).
extern "C" uint32_t ws_utf8_host_text(const unsigned char* body, unsigned long long len, uint32_t state_in,
                                      int continued, int complete, int phase, uint32_t* state_out) {
    const bool hopeless = continued && (state_in & WS_UTF8_ST_FAILED);
    const uint32_t carry3 = continued ? ws_utf8_state_last3(state_in) : 0u;
    uint32_t last3 = carry3, err = 0;
    if (!hopeless && phase < 0) {
        for (unsigned long long i = 0; i < len; ++i) {
            err |= ws_utf8_byte_err(body[i], (last3 >> 16) & 0xFFu, (last3 >> 8) & 0xFFu, last3 & 0xFFu);
            last3 = (last3 >> 8) | (uint32_t)body[i] << 16;
        }
    } else if (!hopeless) {
        const unsigned long long end = (unsigned long long)phase + len, nchunks = (end + 15) / 16;
        uint32_t prev3 = 0;
        for (unsigned long long c = 0; c < nchunks; ++c) {
            unsigned char b[19] = {0};                 // b[3 + j] = chunk byte j, b[0..2] = look-back override
            const unsigned lo = c == 0 ? (unsigned)phase : 0u;
            const unsigned hi = end - 16 * c >= 16 ? 16u : (unsigned)(end - 16 * c);
            for (unsigned j = lo; j < hi; ++j) b[3 + j] = body[16 * c + j - (unsigned)phase];
            if (c == 0)
                for (unsigned j = 0; j < 3; ++j) b[(unsigned)phase + j] = (unsigned char)(carry3 >> (8 * j));
            uint32_t w[4];
            memcpy(w, b + 3, 16);                      // (little-endian hosts)
            const uint32_t look = c == 0 ? (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 : prev3;
            const uint32_t cover = (0xFFFFu >> (16 - hi)) & (0xFFFFu << lo) & 0xFFFFu;
            if (!ws_utf8_chunk_plain(w[0], w[1], w[2], w[3], look))
                err |= ws_utf8_chunk_err(w[0], w[1], w[2], w[3], look) & cover;
            prev3 = ws_utf8_chunk_last3(w[3]);
        }
        for (unsigned long long i = len < 3 ? 0 : len - 3; i < len; ++i) last3 = (last3 >> 8) | (uint32_t)body[i] << 16;
    }
    const uint32_t n = ws_utf8_tail_len((last3 >> 16) & 0xFFu, (last3 >> 8) & 0xFFu, last3 & 0xFFu);
    const bool bad = hopeless || err || (complete && n);
    if (state_out) *state_out = bad ? WS_UTF8_ST_PENDING | WS_UTF8_ST_FAILED : ws_utf8_state_pack(n, last3);
    return bad ? 2u : 1u;
}

// every string of `len` (1..4) bytes over alphabet[0, na), in counting order (the first byte the
// most significant digit), as a fresh complete and a fresh open message: verdict_complete[i],
// verdict_open[i] and state_open[i]
extern "C" void ws_utf8_host_all(const unsigned char* alphabet, unsigned na, unsigned len, int phase,
                                 unsigned char* verdict_complete, unsigned char* verdict_open, uint32_t* state_open) {
    unsigned long long total = 1;
    for (unsigned k = 0; k < len; ++k) total *= na;
    for (unsigned long long i = 0; i < total; ++i) {
        unsigned char s[4];
        unsigned long long r = i;
        for (unsigned k = len; k-- > 0;) {
            s[k] = alphabet[r % na];
            r /= na;
        }
        verdict_complete[i] = (unsigned char)ws_utf8_host_text(s, len, 0, 0, 1, phase, nullptr);
        verdict_open[i] = (unsigned char)ws_utf8_host_text(s, len, 0, 0, 0, phase, state_open + i);
    }
}
