/*
 * wsframe_amd_send.h — a server's outgoing data on the device: every connection's list of
 * messages is fragmented, framed and packed into that connection's wire bytes
 * (libwsframe_amd_send.so: everything libwsframe_amd_reply.so exports plus the entry points below).
 *
 * The reference sends a message by cutting it into packets of the channel's write_fragment_size and
 * framing each packet (net_reactor.c:871-945, websocketframe.c:176-202). This call does that for
 * every message of every connection at once, from bodies that already lie on the device — the
 * output of a reassembly call, for an echo, or one body for many connections — and leaves every
 * connection's bytes back to back, ready for its socket. It is the send-side twin of
 * websocketframeBatchReassembleDevice. Opt-in: no other entry point changes.
 *
 * The rule, with H(n) = websocketframeEncodeHeadLength(n) (+ 4 in the client role) and F the
 * connection's fragment size: shard = F - H(F) (the header length is taken at F, as the reference
 * does: F = 125 gives 123, F = 126 gives 122, F = 65536 gives 65526). A message of L body bytes and
 * opcode T is one frame (FIN, T, empty) when L = 0, else ceil(L / shard) frames of min(shard, what
 * is left) bytes: opcode T on the first and 0 on the others, FIN on the last only, each header
 * websocketframeEncode's for the frame's own length. T is written as given (T & 0x0F). Lengths are
 * 64-bit here and an unsigned int in the reference: the two agree wherever L < 2^32.
 */
#ifndef UTIL_AMD_WSFRAME_AMD_SEND_H
#define UTIL_AMD_WSFRAME_AMD_SEND_H

#include "wsframe_amd_reply.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Entry points of libwsframe_amd_send.so only. */
#define WSFRAME_AMD_SEND_EXPORT __attribute__((visibility("default")))

#define WEBSOCKET_SEND_SKIP 0xFFFFFFFFu   /* WebsocketSendMsg_t.type: the entry emits nothing */
#define WEBSOCKET_SEND_NONE 0xFFFFFFFFu   /* WebsocketSendResult_t.first_bad: no message failed */
#define WEBSOCKET_SEND_FRAG_DEFAULT 0xFFFFFFFFu   /* the reference's write_fragment_size of a stream channel */

/* WebsocketSendResult_t.status */
enum {
    WEBSOCKET_SEND_OK = 0,
    WEBSOCKET_SEND_ERR_FRAGMENT_SIZE = 1, /* F <= H(F) and a message has a body: the reference returns NULL */
    WEBSOCKET_SEND_ERR_RANGE = 2          /* a message's src_off + len > src_len (64-bit)                   */
};

/* One message to send. 24 bytes, 8-B aligned. */
typedef struct WebsocketSendMsg_t {
    unsigned long long src_off, len;     /* body in d_src; ranges may overlap (fan-out) */
    unsigned int type;                   /* opcode of the first frame, or WEBSOCKET_SEND_SKIP */
    unsigned int reserved;               /* 0 */
} WebsocketSendMsg_t;

/* Per-connection result. 32 bytes, 16-B aligned. */
typedef struct WebsocketSendResult_t {
    unsigned long long tx_len;           /* d_tx_off[s+1] - d_tx_off[s] */
    unsigned long long n_frames;         /* frames written for this connection */
    unsigned int n_msgs;                 /* messages sent (entries that are not SKIP) */
    unsigned int status;                 /* WEBSOCKET_SEND_* */
    unsigned int first_bad;              /* index of the first failing message, else WEBSOCKET_SEND_NONE */
    unsigned int reserved;               /* 0 */
} WebsocketSendResult_t;

/* Frame and pack the messages d_msg[s*max_msgs + i], i < min(d_nmsg[s], max_msgs), of every
 * connection s < nseg. Asynchronous, no host synchronisation; may be captured in a HIP graph after
 * one warm call. All grids are sized from nseg, max_msgs and tx_capacity (pass the buffer's real
 * size, not "plenty"); blocks past the device-side total exit at once. An unknown flag (flags is 0),
 * max_msgs == 0, a NULL required pointer (every pointer not marked "may be NULL"; d_tx only when
 * tx_capacity is 0; d_src is required), a misaligned array, src_len > 2^56 or tx_capacity > 2^44
 * returns a negative code (websocketframeGpuLastError) and launches nothing. nseg == 0 writes
 * d_tx_off[0] = 0 only. nseg * max_msgs <= 2^30.
 *
 * Per connection s: F = d_frag_size ? d_frag_size[s] : WEBSOCKET_SEND_FRAG_DEFAULT; the role is the
 * client's when d_mask_key is not NULL. Its entries are taken in order:
 *   - type == WEBSOCKET_SEND_SKIP: nothing is emitted;
 *   - src_off + len > src_len (64-bit): the connection fails with WEBSOCKET_SEND_ERR_RANGE;
 *   - else len > 0 and F <= H(F): the connection fails with WEBSOCKET_SEND_ERR_FRAGMENT_SIZE (an empty
 *     message never looks at F, in the reference as here);
 *   - else the message's frames, by the rule above, follow what the connection has so far.
 * A failed connection sends nothing at all in this call: tx_len, n_frames and n_msgs are 0, status
 * is the first failing message's and first_bad its index.
 * Client role: the MASK bit is set, 4 key bytes follow the length and the body is XORed by byte
 * position. One key per message slot, d_mask_key[s*max_msgs + i], bytes in wire order as
 * WebsocketEncodeDesc_t.mask_key; fragment j of the message uses key ^ (j * 0x9E3779B9) (32-bit),
 * so a message's fragments do not share a key.
 *
 * A connection's frames lie back to back in list order: connection s owns d_tx[d_tx_off[s],
 * d_tx_off[s+1]); d_tx_off is always the full exclusive prefix sum of the connections' lengths, as
 * if tx_capacity were unbounded, and bytes at or past tx_capacity are never written. tx_capacity ==
 * 0 is the sizing call (d_tx may then be NULL). d_msg_tx_off (may be NULL) takes, for every i <
 * min(d_nmsg[s], max_msgs), the first wire byte of message i in d_tx (for an entry that emits
 * nothing: where it would lie); other slots are not written. Nothing but d_tx[0, min(total,
 * tx_capacity)), d_tx_off, d_msg_tx_off, d_send_res and the library's workspace is written; d_src
 * is read only inside the ranges of messages that are sent. d_src and d_tx do not overlap. The sum
 * of all connections' wire bytes must stay below 2^64.
 * d_send_res is 16-B aligned, d_msg, d_tx_off and d_msg_tx_off 8-B, the u32 arrays 4-B; d_src and
 * d_tx may lie anywhere. */
WSFRAME_AMD_SEND_EXPORT int websocketframeBatchSendDevice(
    const unsigned char* d_src, unsigned long long src_len,
    const WebsocketSendMsg_t* d_msg,     /* [s*max_msgs + i], i < d_nmsg[s] */
    const unsigned int* d_nmsg, unsigned int nseg, unsigned int max_msgs,
    const unsigned int* d_frag_size,     /* nseg, may be NULL */
    const unsigned int* d_mask_key,      /* nseg*max_msgs, NULL: server role */
    unsigned int flags,                  /* 0; unknown bits are an error */
    unsigned char* d_tx, unsigned long long tx_capacity,
    unsigned long long* d_tx_off,        /* nseg + 1 */
    unsigned long long* d_msg_tx_off,    /* may be NULL, [s*max_msgs+i]: the message's first wire byte in d_tx */
    WebsocketSendResult_t* d_send_res,   /* nseg */
    void* hip_stream);

/* The send list of an echo, from what a reassembly call on the same stream left behind: a pure map,
 * one thread per slot. Slot s*max_frames + i, i < min(d_nmsg[s], max_frames), becomes {out_off, len,
 * opcode} when message i is complete, not continued, and its first frame's opcode
 * (d_desc[s*max_frames + first_frame].type) is 1 or 2; otherwise a SKIP entry. out_off is taken as
 * it is: WebsocketMsgDesc_t.out_off already counts from d_out, the connection's region offset
 * included. With d_out as d_src, and d_nmsg and max_frames reused as d_nmsg and max_msgs,
 * websocketframeBatchSendDevice then sends every connection its data messages back. Slots at or
 * past d_nmsg[s] are not written. Asynchronous; a NULL pointer or max_frames == 0 returns a
 * negative code; nseg * max_frames <= 2^30. */
WSFRAME_AMD_SEND_EXPORT int websocketframeBatchSendListFromMessagesDevice(
    const WebsocketFrameDesc_t* d_desc, const WebsocketMsgDesc_t* d_msg, const unsigned int* d_nmsg,
    unsigned int nseg, unsigned int max_frames, WebsocketSendMsg_t* d_send_msg, void* hip_stream);

/* The same rule for one connection on the host, for connections that stay on the host path: src[0,
 * src_len) the bodies, msg[0, nmsg) its list, frag_size its F, mask_key (may be NULL: server role)
 * its nmsg keys, tx[0, tx_capacity) the wire bytes, msg_tx_off (may be NULL) nmsg offsets from tx.
 * Returns the full length (bytes at or past tx_capacity are not written; *out says what was
 * built), or a negative code for an unknown flag or a NULL required pointer (msg only when nmsg is
 * 0, tx only when tx_capacity is 0), which leaves *out alone. */
WSFRAME_AMD_SEND_EXPORT long long websocketframeSendHost(
    const unsigned char* src, unsigned long long src_len, const WebsocketSendMsg_t* msg, unsigned int nmsg,
    unsigned int frag_size, const unsigned int* mask_key, unsigned int flags, unsigned char* tx,
    unsigned long long tx_capacity, unsigned long long* msg_tx_off, WebsocketSendResult_t* out);

#ifdef __cplusplus
}
#endif

#endif
