/*
 * wsframe_amd_reply.h — the control frames RFC 6455 obliges an endpoint to send back, built on
 * the device (libwsframe_amd_reply.so: everything libwsframe_amd_hs.so exports plus the entry
 * points below).
 *
 * The decode calls report frames, the protocol check says which close status a connection has
 * earned. This call turns both into bytes for the socket: a PONG for every PING (RFC 6455 5.5.2,
 * 5.5.3), the CLOSE that answers a CLOSE (5.5.1) and the CLOSE that carries the status the
 * protocol check or the caller chose (7.1.7). Its inputs are what the earlier calls left on the
 * device; nothing is copied to the host. Opt-in: no other entry point changes.
 */
#ifndef UTIL_AMD_WSFRAME_AMD_REPLY_H
#define UTIL_AMD_WSFRAME_AMD_REPLY_H

#include "wsframe_amd_handshake.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Entry points of libwsframe_amd_reply.so only. */
#define WSFRAME_AMD_REPLY_EXPORT __attribute__((visibility("default")))

/* which CLOSE a segment's reply ends with */
enum {
    WEBSOCKET_REPLY_CLOSE_NONE = 0,      /* none                                                          */
    WEBSOCKET_REPLY_CLOSE_ECHO = 1,      /* the answer to a received CLOSE: its status, not its reason    */
    WEBSOCKET_REPLY_CLOSE_PROTOCOL = 2,  /* d_proto_res[s].close_status: the peer broke the protocol      */
    WEBSOCKET_REPLY_CLOSE_CALLER = 3     /* d_fail_status[s]: the caller fails the connection             */
};

#define WEBSOCKET_REPLY_WIRE_MASKED    4u  /* same meaning and value as WEBSOCKET_PROTO_WIRE_MASKED: d_buf still
                                              holds masked bodies (after a reassembly call)               */
#define WEBSOCKET_REPLY_LAST_PING_ONLY 8u  /* RFC 6455 5.5.3: answer only the most recent PING              */
#define WEBSOCKET_REPLY_NONE 0xFFFFFFFFu

/* per-connection carry, one u32 per segment, in/out; the caller zeroes it when the connection
   starts. Every other bit is 0. */
#define WEBSOCKET_REPLY_ST_CLOSE_SENT  1u  /* a CLOSE was sent: the connection sends nothing more           */

/* Per-segment result. 16 bytes. */
typedef struct WebsocketReplyResult_t {
    unsigned int n_pong;        /* PONG frames written for this segment                                   */
    unsigned int close_kind;    /* WEBSOCKET_REPLY_CLOSE_*                                                */
    unsigned int close_status;  /* status in the CLOSE sent; 0 when it has no body or none was sent       */
    unsigned int tx_len;        /* d_tx_off[s+1] - d_tx_off[s]                                            */
} WebsocketReplyResult_t;

/* Build the replies to what a decode call (and, optionally, websocketframeBatchCheckProtocolDevice)
 * just produced, on the same stream, descriptors at slots s*max_frames. Asynchronous, no host
 * synchronisation; may be captured in a HIP graph after one warm call. An unknown flag,
 * max_frames == 0 or a NULL required pointer (every pointer not marked "may be NULL"; d_tx only
 * when tx_capacity is 0) returns a negative code (websocketframeGpuLastError) and launches
 * nothing. nseg == 0 writes d_tx_off[0] = 0 only. nseg * max_frames <= 2^30.
 *
 * Per segment s, over the counted frames k < min(d_res[s].n_frames, max_frames) in order; frame k
 * is consumed when ret > 0 and frame_off + ret <= d_seg_off[s] + d_res[s].consumed (64-bit), as
 * in wsframe_amd_proto.h:
 *   - c = the first consumed frame with type 8, else NONE; b = d_proto_res[s].first_bad, NONE when
 *     d_proto_res is NULL; end = min(b, c);
 *   - if the incoming state has CLOSE_SENT nothing is written, the result is all zero and the state
 *     is left alone;
 *   - else the answerable pings are the consumed frames k < end with type 9, is_fin != 0 and
 *     datalen <= 125. Each gets a PONG, in order; with WEBSOCKET_REPLY_LAST_PING_ONLY only the
 *     greatest such k gets one;
 *   - a PONG with T = datalen is the bytes 0x8A, T | (d_mask_key ? 0x80 : 0), the 4 key bytes when
 *     masked, and the ping's unmasked body: d_buf[data_off + i] as is, or, under
 *     WEBSOCKET_REPLY_WIRE_MASKED for a descriptor with `masked`, XORed with d_buf[data_off - 4 +
 *     (i & 3)]; with d_mask_key the body is XORed once more with the reply key's byte i & 3;
 *   - after the pongs at most one CLOSE (0x88, length 0 or 2, masked the same way):
 *       b != NONE and b <= c:                 PROTOCOL, status d_proto_res[s].close_status;
 *       else d_fail_status && d_fail_status[s]: CALLER, status d_fail_status[s] & 0xFFFF;
 *       else c != NONE:                       ECHO: the first two unmasked body bytes of c when its
 *                                             datalen >= 2 (the status is that big-endian u16), else
 *                                             an empty body (status 0). The reason is not echoed.
 *     Status bytes are big-endian. A CLOSE sent sets CLOSE_SENT in the state.
 * d_tx_off is always the full exclusive prefix sum of the segments' reply lengths, as if
 * tx_capacity were unbounded; bytes at or past tx_capacity are never written. A d_tx of
 * 131 B per counted frame plus 8 B per segment always suffices (PONG: 2 + 4 + 125, CLOSE: 2 + 4 + 2).
 * d_buf is read only at the bodies of answered pings, the two status bytes of an echoed CLOSE and
 * their key bytes; nothing but d_tx[0, min(total, tx_capacity)), d_tx_off, d_reply_res,
 * d_reply_state and the library's workspace is written.
 * d_desc, d_res, d_proto_res and d_reply_res are 16-B aligned, d_seg_off and d_tx_off 8-B, the
 * u32 arrays 4-B; d_tx and the bodies in d_buf may lie anywhere. */
WSFRAME_AMD_REPLY_EXPORT int websocketframeBatchControlRepliesDevice(
    const unsigned char* d_buf, const unsigned long long* d_seg_off,
    const WebsocketFrameDesc_t* d_desc, const WebsocketSegResult_t* d_res,
    unsigned int nseg, unsigned int max_frames, unsigned int flags,
    const WebsocketProtoResult_t* d_proto_res, /* nseg, may be NULL: nothing is in error           */
    const unsigned int* d_fail_status,         /* nseg, may be NULL; nonzero: the caller fails this
                                                  connection with this status (1007 from the text
                                                  validator, 1001, ...); low 16 bits are sent      */
    const unsigned int* d_mask_key,            /* NULL: server role, unmasked frames. Else nseg *
                                                  (max_frames+1) keys, wire order as
                                                  WebsocketEncodeDesc_t.mask_key: slot
                                                  s*(max_frames+1)+k masks the PONG answering
                                                  frame k, slot s*(max_frames+1)+max_frames the
                                                  segment's CLOSE                                  */
    unsigned int* d_reply_state,               /* nseg, in/out, may be NULL: every batch alone     */
    unsigned char* d_tx, unsigned long long tx_capacity,
    unsigned long long* d_tx_off,              /* nseg + 1: segment s's reply bytes are
                                                  d_tx[d_tx_off[s], d_tx_off[s+1]); last = total   */
    WebsocketReplyResult_t* d_reply_res,       /* nseg */
    void* hip_stream);

/* The same rule for one segment on the host, for connections that stay on the host path: buf is
 * the buffer desc's offsets point into, seg_off the segment's offset in it, desc / res the
 * segment's max_frames descriptors and its result, proto_res (may be NULL) its protocol result,
 * fail_status as d_fail_status[s], mask_key (may be NULL) the segment's max_frames + 1 keys, state
 * (may be NULL) its carry, tx[0, tx_capacity) the reply. Returns the reply's full length (bytes at
 * or past tx_capacity are not written; *out says what was built), or a negative code for an unknown
 * flag, max_frames == 0 or a NULL required pointer, which leaves *state and *out alone. */
WSFRAME_AMD_REPLY_EXPORT long long websocketframeControlRepliesHost(
    const unsigned char* buf, unsigned long long seg_off, const WebsocketFrameDesc_t* desc,
    const WebsocketSegResult_t* res, unsigned int max_frames, unsigned int flags,
    const WebsocketProtoResult_t* proto_res, unsigned int fail_status, const unsigned int* mask_key,
    unsigned int* state, unsigned char* tx, unsigned long long tx_capacity, WebsocketReplyResult_t* out);

#ifdef __cplusplus
}
#endif

#endif
