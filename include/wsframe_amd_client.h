/*
 * wsframe_amd_client.h — the client side of the opening handshake, batched on the device
 * (libwsframe_amd_cli.so: everything libwsframe_amd_send.so exports plus the entry points below,
 * so one library opens a connection in either role and serves it to its close).
 *
 * Every data-path call can act as the client (the encode masks, the replies and the send take a
 * client role); these two calls open such connections: one builds the upgrade requests of a batch
 * of connections from the reference's two request templates (WEBSOCKET_SIMPLE_HTTP_HANDSHAKE_REQUEST_FMT
 * and ..._WITH_PROTOCOL_FMT of wsframe_amd.h) and the value each server must answer with, the other
 * judges the servers' responses by RFC 6455 section 4.1. Unlike the server side, which restates
 * the reference's parse quirk for quirk, the response is parsed by line with header names compared
 * case-insensitively: the RFC obliges a client to fail the connection unless the checks pass.
 * Opt-in: no other entry point changes.
 */
#ifndef UTIL_AMD_WSFRAME_AMD_CLIENT_H
#define UTIL_AMD_WSFRAME_AMD_CLIENT_H

#include "wsframe_amd_send.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Entry points of libwsframe_amd_cli.so only. */
#define WSFRAME_AMD_CLI_EXPORT __attribute__((visibility("default")))

#define WEBSOCKET_CLI_NONE 0xFFFFFFFFu

/* request descriptor flags */
#define WEBSOCKET_CLI_REQ_WRITTEN  1u   /* req_len bytes were written at the connection's request slot              */
#define WEBSOCKET_CLI_REQ_NO_SPACE 2u   /* req_len > req_cap: no request byte was written (expect is)               */
#define WEBSOCKET_CLI_ERR_RANGE    4u   /* a range does not lie in [0, str_len), the path is empty, or the request
                                           would pass 2^32 - 1 bytes                                                */
#define WEBSOCKET_CLI_ERR_BYTES    8u   /* a byte <= 0x20 or 0x7F in the path, or < 0x20 or 0x7F in the host or the
                                           protocol: no CR or LF can be injected into the request                   */
/* verify descriptor flag */
#define WEBSOCKET_CLI_ERR_SEG_LEN  16u  /* seg_len >= 2^31, or the segment does not lie in [0, buflen): ret -1, the
                                           segment is not read                                                      */

/* WebsocketClientVerifyDesc_t.reason: the first check of RFC 6455 section 4.1 that failed */
enum {
    WEBSOCKET_CLI_OK = 0,
    WEBSOCKET_CLI_REASON_STATUS = 1,      /* the status line is not "HTTP/1.1 101" followed by its end or a space   */
    WEBSOCKET_CLI_REASON_UPGRADE = 2,     /* no Upgrade header, or the first one's value is not "websocket"         */
    WEBSOCKET_CLI_REASON_CONNECTION = 3,  /* no Connection header holds the token "upgrade"                         */
    WEBSOCKET_CLI_REASON_ACCEPT = 4,      /* no Sec-WebSocket-Accept header, or the first one's value is not the 28
                                             expected bytes                                                         */
    WEBSOCKET_CLI_REASON_EXTENSION = 5,   /* a Sec-WebSocket-Extensions header with a value: none was offered       */
    WEBSOCKET_CLI_REASON_PROTOCOL = 6,    /* more than one Sec-WebSocket-Protocol header, or a value that was not
                                             offered                                                                */
    WEBSOCKET_CLI_REASON_TOO_LONG = 7     /* no complete response within max_head bytes                             */
};

/* One connection's strings, as ranges of the string pool d_str[0, str_len). A length of 0 means
 * absent; the path must have path_len >= 1. 48 bytes, 16-B aligned. */
typedef struct WebsocketClientEntry_t {
    unsigned long long path_off;
    unsigned long long proto_off;   /* the offered subprotocols as they go into the header: "a, bb" */
    unsigned long long host_off;
    unsigned int path_len;
    unsigned int proto_len;
    unsigned int host_len;
    unsigned int reserved[3];       /* 0 */
} WebsocketClientEntry_t;

/* Per-connection result of the request call. 16 bytes, written with one 16-B store. */
typedef struct WebsocketClientReqDesc_t {
    unsigned int req_len;    /* bytes of the request; reported even when it did not fit; 0 with an error flag */
    unsigned int key_off;    /* the 24 key characters' offset in the request; 0 with an error flag            */
    unsigned int flags;      /* WEBSOCKET_CLI_REQ_WRITTEN, _REQ_NO_SPACE, _ERR_RANGE, _ERR_BYTES               */
    unsigned int reserved;   /* 0 */
} WebsocketClientReqDesc_t;

/* Per-segment result of the verify call. 32 bytes, 16-B aligned, written with 16-B stores. */
typedef struct WebsocketClientVerifyDesc_t {
    int ret;                 /* > 0 the response passed: bytes up to and including "\r\n\r\n" (frames start
                                there); 0 incomplete; -1 the connection must be failed */
    unsigned int reason;     /* WEBSOCKET_CLI_REASON_* where ret is -1 (0 with WEBSOCKET_CLI_ERR_SEG_LEN), else 0 */
    unsigned int status;     /* the status code of a complete response whose first line starts "HTTP/1.", a
                                digit, a space and three digits (a 302 or a 401 can be read off); else 0 */
    unsigned int proto_off;  /* where ret > 0: the accepted subprotocol's range, from the segment's first byte; */
    unsigned int proto_len;  /* WEBSOCKET_CLI_NONE and 0 when the server named none, and unless ret > 0         */
    unsigned int accept_off; /* of a complete response: the offset of the first Sec-WebSocket-Accept header's
                                value (of its line's end when the value is empty); WEBSOCKET_CLI_NONE when
                                there is no such header, and for an incomplete response */
    unsigned int flags;      /* WEBSOCKET_CLI_ERR_SEG_LEN */
    unsigned int reserved;   /* 0 */
} WebsocketClientVerifyDesc_t;

/* Build every connection's upgrade request. key = the 24 base64 characters of the connection's 16
 * nonce bytes (the caller's random bytes: the device draws none). Without a host the request is
 * exactly what snprintf gives with WEBSOCKET_SIMPLE_HTTP_HANDSHAKE_REQUEST_FMT for (path, key) or,
 * with a protocol, with ..._WITH_PROTOCOL_FMT for (path, key, proto), without the terminating NUL.
 * With a host, "Host: <host>\r\n" follows the request line (the templates have no Host line and
 * most servers refuse HTTP/1.1 without one: an opt-in departure). The request goes to
 * d_req + (d_req_off ? d_req_off[s] : s * req_cap); every other byte of d_req stays untouched.
 * d_expect takes 32 bytes per connection, the 28 characters of base64(SHA-1(key || GUID)) and 4
 * zero bytes (the layout of the server call's d_accept): what the verify call reads. With an
 * error flag nothing is written for the connection but its descriptor; without one, d_expect is
 * written even when the request did not fit.
 *
 * Asynchronous on hip_stream, no host synchronisation, no workspace; may be captured in a HIP
 * graph. nseg == 0 is a no-op; an unknown flag (none is defined: flags must be 0) returns a
 * negative code (websocketframeGpuLastError) and launches nothing. d_entry, d_nonce, d_expect and
 * d_rd are 16-B aligned, d_req_off 8-B aligned; request slots may lie anywhere. */
WSFRAME_AMD_CLI_EXPORT int websocketframeBatchClientRequestDevice(
    const unsigned char* d_str, unsigned long long str_len,
    const WebsocketClientEntry_t* d_entry, const unsigned char* d_nonce /* 16 B per connection */, unsigned int nseg,
    unsigned int flags,
    unsigned char* d_req, const unsigned long long* d_req_off /* optional, NULL = s * req_cap */, unsigned int req_cap,
    unsigned char* d_expect /* 32 B per connection */, WebsocketClientReqDesc_t* d_rd /* nseg */, void* hip_stream);

/* Judge every segment as a server's response. The decode calls' batch contract: segments lie in
 * [0, buflen), WEBSOCKET_BATCH_PAD readable bytes follow every segment, d_buf is only read, and no
 * byte outside a segment influences any result. Asynchronous, no host synchronisation, no
 * workspace; may be captured in a HIP graph. nseg == 0 is a no-op; an unknown flag (flags must be
 * 0) returns a negative code and launches nothing.
 *
 * Completion. T = the first "\r\n\r\n" lying wholly inside the segment. The response is complete
 * iff T exists and (max_head == 0 or T + 4 <= max_head); then e = T. Otherwise max_head != 0 and
 * seg_len >= max_head give ret -1, reason TOO_LONG; otherwise ret 0. No byte at or past max_head
 * influences a result. A NUL byte means nothing special. seg_len == 0 gives ret 0.
 *
 * Lines. [0, e) is cut at every "\r\n"; a bare CR or LF is an ordinary byte. Line 0 is the status
 * line. A later line is a header iff it does not begin with SP or HT and holds a ':' after a
 * non-empty name; the name is everything before the first ':', not trimmed, compared
 * case-insensitively (A-Z folded only); the value is the rest of the line with leading and
 * trailing SP and HT removed.
 *
 * Checks, in the RFC's order; the first that fails sets reason, and ret -1:
 *   STATUS      the status line starts "HTTP/1.1 101" (exact case), and its end or a space follows;
 *   UPGRADE     the first "upgrade" header exists and its value folds to "websocket";
 *   CONNECTION  among all "connection" headers, some comma-separated element, trimmed of SP and
 *               HT, folds to "upgrade";
 *   ACCEPT      the first "sec-websocket-accept" header exists and its value is exactly the 28
 *               bytes d_expect[32 s, 32 s + 28);
 *   EXTENSION   no "sec-websocket-extensions" header has a non-empty value;
 *   PROTOCOL    there is no "sec-websocket-protocol" header, or exactly one, whose value is
 *               non-empty and equals, case-sensitively, one element of the connection's offered
 *               list (d_entry[s]'s proto range, split at ',' and trimmed of SP and HT). With
 *               nothing offered (d_entry NULL, proto_len 0, or a range outside the pool, which is
 *               not read) such a header fails.
 * All pass: ret = e + 4.
 *
 * d_cv and d_expect are 16-B aligned, d_entry (optional, with d_str) 16-B aligned, d_seg_off /
 * d_seg_len 8-B aligned. */
WSFRAME_AMD_CLI_EXPORT int websocketframeBatchClientVerifyDevice(
    const unsigned char* d_buf, unsigned long long buflen,
    const unsigned long long* d_seg_off, const unsigned long long* d_seg_len, unsigned int nseg,
    unsigned int flags,
    const unsigned char* d_expect,            /* 32 B per segment, as the request call wrote them */
    const unsigned char* d_str, unsigned long long str_len,
    const WebsocketClientEntry_t* d_entry,    /* optional: NULL = nothing was offered */
    unsigned int max_head,
    WebsocketClientVerifyDesc_t* d_cv,        /* nseg */
    void* hip_stream);

/* The same rules for one connection that stays on the host path. The request call: req (optional)
 * takes req_len bytes when they fit in req_cap, expect 32 bytes, *rd the descriptor. Returns 0, or
 * a negative code for an unknown flag or a NULL rd, expect or nonce (and writes nothing). */
WSFRAME_AMD_CLI_EXPORT int websocketframeClientRequestHost(
    const unsigned char* path, unsigned int path_len, const unsigned char* proto, unsigned int proto_len,
    const unsigned char* host, unsigned int host_len, const unsigned char nonce[16], unsigned int flags,
    unsigned char* req, unsigned int req_cap, unsigned char expect[32], WebsocketClientReqDesc_t* rd);

/* buf[0, len) with WEBSOCKET_BATCH_PAD readable bytes after it; offered (optional) is the offered
 * subprotocol list. Returns 0, or a negative code for an unknown flag or a NULL cv or expect (and
 * leaves *cv alone). */
WSFRAME_AMD_CLI_EXPORT int websocketframeClientVerifyHost(
    const unsigned char* buf, unsigned int len, unsigned int flags, const unsigned char expect[32],
    const unsigned char* offered, unsigned int offered_len, unsigned int max_head, WebsocketClientVerifyDesc_t* cv);

#ifdef __cplusplus
}
#endif

#endif
