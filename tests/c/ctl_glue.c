/*
 * ctl_glue.c — TEST INFRASTRUCTURE ONLY (dev container): the RFC 6455 5.4 glue a user of the
 * reference writes, around the REFERENCE's own websocketframeDecode (oracle/_ref/libwsref.so):
 * the websocket glue of SURVEY §8b, but a control frame (type & 8) keeps pktype = 0, so the
 * stream hook hands it straight to on_recv (net_channel_ex.c:125-126, 155). Built into
 * oracle/_ref/libctl_glue.so by tests/golden/make_reasm_ctl_golden.py and registered as
 * NetChannelExProc_t.on_decode of the reference reactor (tests/ref_reactor.py); it pins the
 * rule of WEBSOCKET_REASM_CONTROL_DIRECT in tests/golden/reassemble_ctl.json.
 */
#include "wsframe_amd_channel.h"

void ctl_glue_on_decode(struct NetChannel_t* channel, unsigned char* buf, size_t len,
                        struct NetChannelInbufDecodeResult_t* result) {
    WebsocketInbufDecodeResult_t* r = (WebsocketInbufDecodeResult_t*)result;
    unsigned char* data = 0;
    unsigned long long datalen = 0;
    int is_fin = 0, type = 0;
    int ret = websocketframeDecode(buf, (unsigned long long)len, &data, &datalen, &is_fin, &type);
    (void)channel;
    if (ret < 0) { r->err = 1; return; }
    if (ret == 0) { r->incomplete = 1; return; }
    r->decodelen = (unsigned int)ret;
    r->bodyptr = data;
    r->bodylen = (unsigned int)datalen;
    r->fragment_eof = (char)is_fin;
    r->pktype = (type & 8) ? 0 : WEBSOCKET_NETPACKET_FRAGMENT;
}
