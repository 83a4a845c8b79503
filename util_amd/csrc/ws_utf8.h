// ws_utf8.h — the UTF-8 rule of the text validator (RFC 3629 as RFC 6455 5.6 / 8.1 asks for
// it), defined once: what a byte means given the three bytes before it, what counts as an
// unfinished tail, and how the per-connection state word is packed. Plain C++ — no HIP header,
// no AMDGPU builtin — so the kernel (ws_utf8.hip) and a host driver (tests/c/utf8_host.cpp,
// tests/test_text_host.py) build the same text and cannot drift apart.
//
// Look-back form. A byte b with the bytes p1 (just before it), p2, p3 before it is in error iff
//   - it is C0, C1 or F5..FF, or
//   - a lead among p1..p3 claims it (p1 >= C0, p2 >= E0 or p3 >= F0) and it is no continuation
//     byte (80..BF), or
//   - no lead claims it and it is a continuation byte, or
//   - it is claimed by p1 (the second byte of a sequence) and lies outside p1's range:
//     E0 takes A0..BF, ED 80..9F, F0 90..BF, F4 80..8F.
// "No byte" before the start of a string is 0x00: an ASCII byte claims nothing. Up to the first
// byte in error of a string this rule says what the sequential decoder says, and past it nothing
// matters: a string is well formed iff no byte is in error and nothing is left unfinished at its
// end, and it is a prefix of a well-formed string iff no byte is in error.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define WS_UTF8_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define WS_UTF8_FN static inline
#endif

// the per-connection carry word (include/wsframe_amd_text.h: WEBSOCKET_TEXT_ST_*)
#define WS_UTF8_ST_PENDING 0x80000000u
#define WS_UTF8_ST_FAILED 0x40000000u

// does a lead among the three bytes before it claim the next byte as a continuation byte?
WS_UTF8_FN uint32_t ws_utf8_claims(uint32_t p1, uint32_t p2, uint32_t p3) {
    return (uint32_t)((p1 >= 0xC0u) | (p2 >= 0xE0u) | (p3 >= 0xF0u));
}

// 1 if byte b is in error after p3 p2 p1 (p1 nearest)
WS_UTF8_FN uint32_t ws_utf8_byte_err(uint32_t b, uint32_t p1, uint32_t p2, uint32_t p3) {
    const uint32_t cont = (uint32_t)((b & 0xC0u) == 0x80u);
    uint32_t err = (uint32_t)((b == 0xC0u) | (b == 0xC1u) | (b >= 0xF5u));
    err |= ws_utf8_claims(p1, p2, p3) ^ cont;
    err |= (uint32_t)(((p1 == 0xE0u) & (b < 0xA0u)) | ((p1 == 0xEDu) & (b > 0x9Fu)) | ((p1 == 0xF0u) & (b < 0x90u)) |
                      ((p1 == 0xF4u) & (b > 0x8Fu)));
    return err;
}

// Length 0..3 of the unfinished sequence at the end of a string without a byte in error whose
// last three bytes are p3 p2 p1: the shortest suffix whose removal leaves a well-formed string.
WS_UTF8_FN uint32_t ws_utf8_tail_len(uint32_t p1, uint32_t p2, uint32_t p3) {
    return p1 >= 0xC0u ? 1u : (p2 >= 0xE0u ? 2u : (p3 >= 0xF0u ? 3u : 0u));
}

// State word of a pending text message: its n-byte tail, first byte in bits 0-7.
// last3 = p3 | p2 << 8 | p1 << 16 (the last three bytes in string order).
WS_UTF8_FN uint32_t ws_utf8_state_pack(uint32_t n, uint32_t last3) {
    const uint32_t bytes = n ? (last3 & 0xFFFFFFu) >> (8u * (3u - n)) : 0u;
    return WS_UTF8_ST_PENDING | (n << 24) | bytes;
}
WS_UTF8_FN uint32_t ws_utf8_state_n(uint32_t st) { return (st >> 24) & 3u; }
// The carried bytes as the three bytes before a continued body's first byte, p3 | p2 << 8 |
// p1 << 16, "no byte" where the tail is shorter. A word without PENDING, or FAILED, carries none.
WS_UTF8_FN uint32_t ws_utf8_state_last3(uint32_t st) {
    if (!(st & WS_UTF8_ST_PENDING) || (st & WS_UTF8_ST_FAILED)) return 0u;
    const uint32_t n = ws_utf8_state_n(st);
    return n ? ((st & 0xFFFFFFu) << (8u * (3u - n))) & 0xFFFFFFu : 0u;
}

// Error bits (bit j = byte j) of the 16 bytes w0..w3 (little-endian dwords) that follow the
// three bytes last3 = p3 | p2 << 8 | p1 << 16.
WS_UTF8_FN uint32_t ws_utf8_chunk_err(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t last3) {
    uint32_t p3 = last3 & 0xFFu, p2 = (last3 >> 8) & 0xFFu, p1 = (last3 >> 16) & 0xFFu, bits = 0;
    const uint32_t w[4] = {w0, w1, w2, w3};
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int j = 0; j < 16; ++j) {
        const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        bits |= ws_utf8_byte_err(b, p1, p2, p3) << j;
        p3 = p2; p2 = p1; p1 = b;
    }
    return bits;
}
// the last three bytes of the 16 (p3 | p2 << 8 | p1 << 16): what the next chunk looks back at
WS_UTF8_FN uint32_t ws_utf8_chunk_last3(uint32_t w3) { return w3 >> 8; }
// a chunk of ASCII bytes after a string that leaves nothing unfinished has no byte in error
WS_UTF8_FN uint32_t ws_utf8_chunk_plain(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t last3) {
    return (uint32_t)((((w0 | w1 | w2 | w3) & 0x80808080u) == 0u) &
                      !ws_utf8_claims((last3 >> 16) & 0xFFu, (last3 >> 8) & 0xFFu, last3 & 0xFFu));
}
