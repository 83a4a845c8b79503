// util_amd/csrc/ws_inflate.h compiled for the host: the connection walk as a C function for ctypes
// (tests/test_inflate_host.py) and, with -DINFLATE_HOST_MAIN, a program of its own that runs a file
// of cases with every buffer allocated at exactly its stated length (the sanitizer build).
#include "../../util_amd/csrc/ws_inflate.h"

extern "C" long long ws_inflate_host_connection(const unsigned char* src, unsigned long long src_len,
                                                const WebsocketInflateMsg_t* msg, unsigned int nmsg,
                                                unsigned long long limit, unsigned char* dst, unsigned long long dst_cap,
                                                WebsocketInflateMsgRes_t* msg_res, WebsocketInflateResult_t* out) {
    return (long long)ws_inflate_connection(src, src_len, msg, nmsg, limit, dst, dst_cap, msg_res, out);
}

// sizeof and alignof of the three records and of the table structs
extern "C" void ws_inflate_host_sizes(unsigned int* v) {
    v[0] = sizeof(WebsocketInflateMsg_t); v[1] = alignof(WebsocketInflateMsg_t);
    v[2] = sizeof(WebsocketInflateMsgRes_t); v[3] = alignof(WebsocketInflateMsgRes_t);
    v[4] = sizeof(WebsocketInflateResult_t); v[5] = alignof(WebsocketInflateResult_t);
    v[6] = sizeof(WsInfTabs); v[7] = sizeof(WsInfWork);
}

#ifdef INFLATE_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// file: u32 ncases, then per case u32 {src_len, limit, cap, status, out_len}, the body, the expected output
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned int ncase = 0;
    if (fread(&ncase, 4, 1, f) != 1) return 2;
    for (unsigned int c = 0; c < ncase; ++c) {
        unsigned int h[5];
        if (fread(h, 4, 5, f) != 5) return 2;
        unsigned char* src = (unsigned char*)malloc(h[0]);       // exactly as long as they are said to be
        unsigned char* want = (unsigned char*)malloc(h[4]);
        unsigned char* dst = (unsigned char*)malloc(h[2]);
        if (h[0] && fread(src, 1, h[0], f) != h[0]) return 2;
        if (h[4] && fread(want, 1, h[4], f) != h[4]) return 2;
        WebsocketInflateMsg_t* m = (WebsocketInflateMsg_t*)malloc(sizeof(WebsocketInflateMsg_t));
        m->src_off = 0; m->len = h[0]; m->kind = WEBSOCKET_INFLATE_RAW; m->reserved = 0;
        WebsocketInflateMsgRes_t* r = (WebsocketInflateMsgRes_t*)malloc(sizeof(WebsocketInflateMsgRes_t));
        WebsocketInflateResult_t out;
        ws_inflate_connection(src, h[0], m, 1, h[1], dst, h[2], r, &out);
        if (out.status != h[3] || r->status != h[3] || out.out_len != h[4] || (h[4] && memcmp(dst, want, h[4]))) {
            printf("case %u: status %u (expected %u), length %llu (expected %u)\n", c, out.status, h[3], out.out_len, h[4]);
            return 1;
        }
        free(src); free(want); free(dst); free(m); free(r);
    }
    fclose(f);
    printf("inflate_host ok: %u cases\n", ncase);
    return 0;
}
#endif
