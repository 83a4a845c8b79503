/*
 * wsframe_amd_handshake.h — the server side of the opening handshake, batched on the device
 * (libwsframe_amd_hs.so: everything libwsframe_amd_proto.so exports plus the entry points below,
 * so one library serves a connection from its upgrade request to its close).
 *
 * A channel that has not upgraded yet holds an HTTP request in its inbuf. In the batch binding
 *  those bytes lie in the device batch next to every other channel's; this call
 * does for them what websocketframeDecodeHandshakeRequest, websocketframeComputeSecAccept and
 * websocketframeEncodeHandshakeResponse[WithProtocol] do one connection at a time, bit for bit,
 * the reference's quirks included (nothing is validated that the reference does not validate).
 * Opt-in: no other entry point changes.
 */
#ifndef UTIL_AMD_WSFRAME_AMD_HANDSHAKE_H
#define UTIL_AMD_WSFRAME_AMD_HANDSHAKE_H

#include "wsframe_amd_proto.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Entry points of libwsframe_amd_hs.so only. */
#define WSFRAME_AMD_HS_EXPORT __attribute__((visibility("default")))

#define WEBSOCKET_HS_NONE 0xFFFFFFFFu

/* descriptor flags */
#define WEBSOCKET_HS_RESP_WRITTEN  1u   /* resp_len bytes were written at the segment's response slot            */
#define WEBSOCKET_HS_RESP_NO_SPACE 2u   /* resp_len > resp_cap: nothing was written                               */
#define WEBSOCKET_HS_ERR_SEG_LEN   4u   /* seg_len >= 2^31 (the reference's int return cannot express it), or the
                                           segment does not lie in [0, buflen): ret -1, the segment is not read   */

/* call flags */
#define WEBSOCKET_HS_ECHO_PROTOCOL 1u   /* the response echoes the parsed Sec-WebSocket-Protocol range, as
                                           websocketframeEncodeHandshakeResponseWithProtocol would                */

/* Per-segment result. 32 bytes, 16-B aligned, written with 16-B stores. */
typedef struct WebsocketHandshakeDesc_t {
    int ret;                 /* websocketframeDecodeHandshakeRequest's return for (buf + seg_off, seg_len):
                                > 0 bytes up to and including "\r\n\r\n" (frames start there), 0 incomplete,
                                -1 error */
    unsigned int key_off;    /* from the segment's first byte; 0 unless ret > 0 */
    unsigned int key_len;
    unsigned int proto_off;  /* WEBSOCKET_HS_NONE where the reference leaves *sec_protocol NULL, and unless ret > 0 */
    unsigned int proto_len;
    unsigned int resp_len;   /* bytes of the response (0 unless ret > 0): 129, or 155 + proto_len with
                                WEBSOCKET_HS_ECHO_PROTOCOL and a parsed protocol; reported even when it did not
                                fit and when no response buffer was given */
    unsigned int flags;      /* WEBSOCKET_HS_RESP_WRITTEN, WEBSOCKET_HS_RESP_NO_SPACE, WEBSOCKET_HS_ERR_SEG_LEN */
    unsigned int reserved;   /* 0 */
} WebsocketHandshakeDesc_t;

/* Parse every segment as an upgrade request, compute Sec-WebSocket-Accept and write the 101
 * response. The decode calls' batch contract: segments lie in [0, buflen), WEBSOCKET_BATCH_PAD
 * readable bytes follow every segment, d_buf is only read, and no byte outside a segment
 * influences any result. Asynchronous, no host synchronisation, no workspace; may be captured in
 * a HIP graph. nseg == 0 is a no-op; an unknown flag returns a negative code
 * (websocketframeGpuLastError) and launches nothing.
 *
 * Per segment, with (data, datalen) = (d_buf + d_seg_off[s], d_seg_len[s]), exactly the reference:
 *   - e = the first "\r\n\r\n" lying wholly inside the segment with no NUL byte before it; none: ret 0;
 *   - the first "Sec-WebSocket-Key:" wholly inside [0, e) (case-sensitive, anywhere, the request
 *     line included); none: ret -1. Its value starts after every following byte that is <= 32 as a
 *     signed char (bytes >= 0x80 are skipped too, and the skip runs over "\r\n" into the next
 *     line); a skip that reaches e: ret -1. The value ends at the first '\r' at or before e;
 *   - the first "Sec-WebSocket-Protocol:" likewise; none, or a skip that reaches e: absent;
 *   - ret = e + 4.
 * Where ret > 0: accept = base64(SHA-1(key || GUID)) for any key length, and the response is
 * websocketframeEncodeHandshakeResponse(accept, 28, ...) or, with WEBSOCKET_HS_ECHO_PROTOCOL,
 * ...WithProtocol(accept, 28, the parsed protocol range), without the terminating NUL: exactly
 * resp_len bytes at d_resp + (d_resp_off ? d_resp_off[s] : s * resp_cap), every other byte of d_resp
 * untouched. seg_len == 0 gives ret 0.
 *
 * d_hs and d_accept are 16-B aligned, d_seg_off / d_seg_len / d_resp_off 8-B aligned; d_resp slots
 * may lie anywhere (16-B and dword stores are used where a slot's address allows). */
WSFRAME_AMD_HS_EXPORT int websocketframeBatchHandshakeDevice(
    const unsigned char* d_buf, unsigned long long buflen,
    const unsigned long long* d_seg_off, const unsigned long long* d_seg_len, unsigned int nseg,
    unsigned int flags,
    WebsocketHandshakeDesc_t* d_hs,   /* nseg */
    unsigned char* d_accept,          /* optional: 32 B per segment, 28 accept characters + 4 zero bytes,
                                         written only where ret > 0 */
    unsigned char* d_resp,            /* optional: NULL = parse and accept only */
    const unsigned long long* d_resp_off, /* optional, NULL = s * resp_cap */
    unsigned int resp_cap, void* hip_stream);

/* The same rule for one segment, for connections that stay on the host path. buf[0, len) with
 * WEBSOCKET_BATCH_PAD readable bytes after it; accept (optional) takes 32 bytes where ret > 0; resp
 * (optional) takes resp_len bytes when they fit in resp_cap. Returns 0, or a negative code for an
 * unknown flag or a NULL hs (and leaves *hs alone). */
WSFRAME_AMD_HS_EXPORT int websocketframeHandshakeHost(const unsigned char* buf, unsigned int len, unsigned int flags,
                                                      WebsocketHandshakeDesc_t* hs, unsigned char accept[32],
                                                      unsigned char* resp, unsigned int resp_cap);

#ifdef __cplusplus
}
#endif

#endif
