// The reactor loop over one rx segment, one candidate at a time, through the kernels' own step
// rule (ws_parse + ws_cand_code of util_amd/csrc/ws_step.h) compiled for the host:
// tests/test_step_host.py holds it against the oracle. No unmask.
#include <string.h>

#include "../../util_amd/csrc/ws_step.h"

// buf[0, buf_bytes) holds the wire; the segment is [seg_off, seg_off + seg_len) of it. Header
// bytes are taken as the kernels get them: the 16 bytes from the candidate on as two
// little-endian u64, whatever lies after the segment included (past the buffer: zeros).
extern "C" void ws_step_host_segment(const unsigned char* buf, u64 buf_bytes, u64 seg_off, u64 seg_len,
                                     u32 max_frames, WebsocketFrameDesc_t* desc, WebsocketSegResult_t* res) {
    u64 off = 0;
    u32 nf = 0;
    int status = WEBSOCKET_SEG_OK;
    for (;;) {
        const bool eval = off < seg_len;
        const u64 at = seg_off + (eval ? off : 0);
        unsigned char b[16] = {0};
        if (at < buf_bytes) memcpy(b, buf + at, buf_bytes - at < 16 ? buf_bytes - at : 16);
        u64 h0 = 0, h1 = 0;
        for (int i = 7; i >= 0; --i) {
            h0 = (h0 << 8) | b[i];
            h1 = (h1 << 8) | b[8 + i];
        }
        const WsHdr h = ws_parse(h0, h1, eval ? seg_len - off : 0);
        const u32 code = ws_cand_code(off, seg_len, nf, max_frames, h, 0, true, status);
        if (code == 3) break;
        if (h.ret != 0) {                                              // a ret == 0 frame has no descriptor
            WebsocketFrameDesc_t* d = desc + nf++;
            d->frame_off = seg_off + off;
            d->data_off = h.plen ? seg_off + off + h.hdr : WEBSOCKET_DATA_OFF_NULL;
            d->datalen = h.plen;
            d->ret = h.ret;
            d->is_fin = (unsigned char)(h.b0 >> 7);
            d->type = (unsigned char)(h.b0 & 0x0Fu);
            d->masked = (unsigned char)h.masked;
            d->hdrlen = (unsigned char)h.hdr;
        }
        if (code == 2) break;
        off += (u32)h.ret;
    }
    res->consumed = off;
    res->n_frames = nf;
    res->status = status;
}
