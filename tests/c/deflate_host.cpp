// util_amd/csrc/ws_deflate.h compiled for the host: the list walk as a C function for ctypes
// (tests/test_deflate_host.py) and, with -DDEFLATE_HOST_MAIN, a program of its own that runs a file
// of cases with every buffer allocated at exactly its stated length (the sanitizer build) and
// inflates every DEFLATED body again with util_amd/csrc/ws_inflate.h.
#include "../../util_amd/csrc/ws_deflate.h"
#include "../../util_amd/csrc/ws_inflate.h"

extern "C" long long ws_deflate_host_list(const unsigned char* src, unsigned long long src_len, const WebsocketDeflateMsg_t* msg,
                                          unsigned int nmsg, unsigned long long min_len, unsigned char* dst,
                                          const unsigned long long* dst_off, const unsigned long long* dst_cap,
                                          WebsocketDeflateMsgRes_t* msg_res, unsigned long long* enc_len) {
    return (long long)ws_deflate_list(src, src_len, msg, nmsg, min_len, dst, dst_off, dst_cap, msg_res, enc_len);
}

// a send-list entry from an entry's type and its result
extern "C" void ws_deflate_host_send_entry(unsigned int type, const WebsocketDeflateMsgRes_t* r, WebsocketSendMsg_t* out) {
    *out = ws_deflate_send_entry(type, *r);
}

// sizeof and alignof of the records and of the scratch, the rule's constants
extern "C" void ws_deflate_host_sizes(unsigned int* v) {
    v[0] = sizeof(WebsocketDeflateMsg_t); v[1] = alignof(WebsocketDeflateMsg_t);
    v[2] = sizeof(WebsocketDeflateMsgRes_t); v[3] = alignof(WebsocketDeflateMsgRes_t);
    v[4] = sizeof(WsDefWork); v[5] = WS_DEF_GROUP; v[6] = WS_DEF_MINMATCH; v[7] = WS_DEF_HBITS_MAX;
}

#ifdef DEFLATE_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// file: u32 ncases, then per case u32 {len, min_len, cap}, the body
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned int ncase = 0, count[5] = {0, 0, 0, 0, 0};
    if (fread(&ncase, 4, 1, f) != 1) return 2;
    for (unsigned int c = 0; c < ncase; ++c) {
        unsigned int h[3];
        if (fread(h, 4, 3, f) != 3) return 2;
        unsigned char* src = (unsigned char*)malloc(h[0]);       // exactly as long as they are said to be
        unsigned char* dst = (unsigned char*)malloc(h[2]);
        unsigned char* back = (unsigned char*)malloc(h[0]);
        if (h[0] && fread(src, 1, h[0], f) != h[0]) return 2;
        WebsocketDeflateMsg_t* m = (WebsocketDeflateMsg_t*)malloc(sizeof(WebsocketDeflateMsg_t));
        m->src_off = 0; m->len = h[0]; m->type = 2; m->reserved = 0;
        WebsocketDeflateMsgRes_t* r = (WebsocketDeflateMsgRes_t*)malloc(sizeof(WebsocketDeflateMsgRes_t));
        unsigned long long off = 0, cap = h[2], enc = 0;
        ws_deflate_list(src, h[0], m, 1, h[1], dst, &off, &cap, r, &enc);
        const bool coded = h[0] && h[0] >= h[1];
        unsigned int want = WEBSOCKET_DEFLATE_ERR_OUT_SPACE;
        if (coded && enc < h[0] && enc <= cap) want = WEBSOCKET_DEFLATE_DEFLATED;
        else if (h[0] <= cap) want = WEBSOCKET_DEFLATE_PLAIN;
        bool ok = r->status == want && r->out_off == 0 && (coded || enc == 0);
        if (ok && want == WEBSOCKET_DEFLATE_DEFLATED) {
            WebsocketInflateMsg_t im = {0, r->out_len, WEBSOCKET_INFLATE_RAW, 0};
            WebsocketInflateMsgRes_t ir;
            WebsocketInflateResult_t io;
            ws_inflate_connection(dst, r->out_len, &im, 1, 0, back, h[0], &ir, &io);
            ok = r->out_len == enc && io.status == WEBSOCKET_INFLATE_OK && io.out_len == h[0] && !memcmp(back, src, h[0]);
        } else if (ok && want == WEBSOCKET_DEFLATE_PLAIN) {
            ok = r->out_len == h[0] && (!h[0] || !memcmp(dst, src, h[0]));
        } else if (ok) {
            ok = r->out_len == 0;
        }
        if (!ok) {
            printf("case %u: len %u min_len %u cap %u: status %u (expected %u), out_len %llu, enc_len %llu\n", c, h[0], h[1], h[2],
                   r->status, want, r->out_len, enc);
            return 1;
        }
        ++count[r->status];
        free(src); free(dst); free(back); free(m); free(r);
    }
    fclose(f);
    printf("deflate_host ok: %u cases, %u deflated, %u plain, %u out of space\n", ncase, count[0], count[1], count[3]);
    return 0;
}
#endif
