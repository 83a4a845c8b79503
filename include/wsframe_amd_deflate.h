/*
 * wsframe_amd_deflate.h — the receive side of RFC 7692 permessage-deflate on the device: every
 * connection's compressed messages are inflated into that connection's output region
 * (libwsframe_amd_deflate.so: everything libwsframe_amd_cli.so exports plus the entry points below).
 *
 * A message whose first frame carries RSV1 is a raw DEFLATE stream (RFC 1951) with its last four
 * bytes, 00 00 FF FF, taken off (RFC 7692 section 7.2.1). These calls put the bytes back — virtually:
 * nothing is read behind the body and the source is never written — and inflate the message with
 * no window from earlier messages, which is what a server gets when it answers the offer with
 * client_no_context_takeover (section 7.1.1.1). Opt-in: no other entry point changes.
 *
 * The rule (util_amd/csrc/ws_inflate.h, one definition for the kernel, the host entry point and the
 * CPU test): a message's input is its body followed by 00 00 FF FF; its output is what zlib's raw
 * inflate (windowBits -15) yields from that input. A symbol counts only when all its bits are
 * present (a literal code; a length code, its extra bits, the distance code and its extra bits; a
 * stored block's LEN and NLEN); a stored block copies as many of its bytes as the input holds; input
 * that runs out anywhere is not an error: the output so far is the message. After a block with
 * BFINAL = 1 decoding stops and what follows is ignored. The message is in error
 * (WEBSOCKET_INFLATE_ERR_DATA) exactly where zlib raises: block type 3; a stored LEN != ~NLEN;
 * HLIT > 286 or HDIST > 30 symbols; a repeat code with nothing to repeat or one that runs past
 * HLIT + HDIST; no code for symbol 256; an over-subscribed or incomplete code-length set; an
 * over-subscribed literal/length or distance set; an incomplete one other than a single code of
 * length 1; a literal/length symbol 286 or 287 or a distance symbol 30 or 31; a code that is not in
 * an incomplete set; a distance farther back than the message's own output so far.
 *
 * Limits, in decode order, as zlib with room for max_message_size + 1 bytes (0: no limit): a symbol
 * is first judged (ERR_DATA; a match's distance only while room is left); then, if it needs a byte
 * beyond those, decoding stops and the message is WEBSOCKET_INFLATE_ERR_TOO_BIG — an error behind that
 * point is never seen, one that needs no further output byte to be reached still is. A message that
 * ends with more than max_message_size bytes is ERR_TOO_BIG. A message that passes both checks to
 * its end but does not fit into what is left of the connection's room is
 * WEBSOCKET_INFLATE_ERR_OUT_SPACE (it is decoded to its end without being written, so an error or
 * the limit anywhere in it still wins).
 */
#ifndef UTIL_AMD_WSFRAME_AMD_DEFLATE_H
#define UTIL_AMD_WSFRAME_AMD_DEFLATE_H

#include "wsframe_amd_client.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Entry points of libwsframe_amd_deflate.so only. */
#define WSFRAME_AMD_DEFLATE_EXPORT __attribute__((visibility("default")))

#define WEBSOCKET_INFLATE_SKIP 0xFFFFFFFFu   /* WebsocketInflateMsg_t.kind: the entry does nothing */
#define WEBSOCKET_INFLATE_RAW  1u            /* a permessage-deflate body, no context */
#define WEBSOCKET_INFLATE_NONE 0xFFFFFFFFu   /* WebsocketInflateResult_t.first_bad: no entry failed */

/* WebsocketInflateMsgRes_t.status and WebsocketInflateResult_t.status */
enum {
    WEBSOCKET_INFLATE_OK = 0,
    WEBSOCKET_INFLATE_ERR_DATA = 1,      /* not a DEFLATE stream (the rule above): close status 1007          */
    WEBSOCKET_INFLATE_ERR_TOO_BIG = 2,   /* the message passes max_message_size: close status 1009           */
    WEBSOCKET_INFLATE_ERR_OUT_SPACE = 3, /* the message does not fit into the connection's room: close_status 0 */
    WEBSOCKET_INFLATE_ERR_RANGE = 4,     /* src_off + len > src_len (64-bit), or an unknown kind: close_status 0 */
    WEBSOCKET_INFLATE_NOT_RUN = 5        /* an entry after the connection's first failure (per message only)  */
};

/* One message to inflate. 24 bytes, 8-B aligned. */
typedef struct WebsocketInflateMsg_t {
    unsigned long long src_off, len;     /* the compressed body in d_src */
    unsigned int kind;                   /* WEBSOCKET_INFLATE_RAW or WEBSOCKET_INFLATE_SKIP */
    unsigned int reserved;               /* 0 */
} WebsocketInflateMsg_t;

/* Per-message result. 24 bytes, 8-B aligned. */
typedef struct WebsocketInflateMsgRes_t {
    unsigned long long out_off;          /* the message's first output byte, counted from d_dst */
    unsigned long long out_len;          /* its inflated length; 0 unless status is OK */
    unsigned int status;                 /* WEBSOCKET_INFLATE_* */
    unsigned int reserved;               /* 0 */
} WebsocketInflateMsgRes_t;

/* Per-connection result. 24 bytes, 8-B aligned. */
typedef struct WebsocketInflateResult_t {
    unsigned long long out_len;          /* bytes of the messages that stand, back to back from d_dst + d_dst_off[s] */
    unsigned int n_msgs;                 /* RAW entries inflated (before the first failure) */
    unsigned int status;                 /* WEBSOCKET_INFLATE_OK, or the first failing entry's status */
    unsigned int first_bad;              /* its index, else WEBSOCKET_INFLATE_NONE */
    unsigned int close_status;           /* 1007 for ERR_DATA, 1009 for ERR_TOO_BIG, else 0 */
} WebsocketInflateResult_t;

/* Inflate the entries d_msg[s*max_msgs + i], i < min(d_nmsg[s], max_msgs), of every connection
 * s < nseg, in order. Asynchronous, no host synchronisation; may be captured in a HIP graph after one
 * warm call. All grids are sized from nseg and max_msgs. An unknown flag (flags is 0), max_msgs == 0,
 * a NULL pointer, a misaligned array or nseg * max_msgs > 2^30 returns a negative code
 * (websocketframeGpuLastError) and launches nothing. nseg == 0 does nothing.
 *
 * Connection s owns d_dst[d_dst_off[s], d_dst_off[s] + d_dst_cap[s]): its room. Its messages'
 * outputs lie back to back from the room's first byte, in list order. Per entry, d_msg_res takes
 * out_off (counted from d_dst: where the entry's output lies, or would lie), out_len and status:
 *   - kind == WEBSOCKET_INFLATE_SKIP: status OK, out_len 0, nothing is read or written;
 *   - src_off + len > src_len (64-bit), or a kind that is neither RAW nor SKIP: ERR_RANGE;
 *   - else the message is inflated by the rule above, with max_message_size and what is left of
 *     the room as its limits.
 * The first failing entry ends the connection: d_res[s] takes its status, its index as first_bad
 * and close_status; the entry's own out_len is 0 and every later entry i < min(d_nmsg[s], max_msgs)
 * gets WEBSOCKET_INFLATE_NOT_RUN with out_off where the failing entry's output would lie and
 * out_len 0. The messages before it stand: d_res[s].n_msgs and out_len count them only. Slots at or
 * past min(d_nmsg[s], max_msgs) are not written.
 *
 * Inside a connection's room the bytes past its out_len are unspecified (a failing message may
 * have written part of its output there). Nothing but the rooms, d_msg_res and d_res is written
 * (the call needs no workspace); d_src is read only inside the ranges of RAW entries. The rooms do
 * not overlap each other or d_src. d_msg, d_msg_res, d_res, d_dst_off and d_dst_cap are 8-B
 * aligned, d_nmsg 4-B; d_src and d_dst may lie anywhere. */
WSFRAME_AMD_DEFLATE_EXPORT int websocketframeBatchInflateDevice(
    const unsigned char* d_src, unsigned long long src_len,
    const WebsocketInflateMsg_t* d_msg,  /* [s*max_msgs + i], i < d_nmsg[s] */
    const unsigned int* d_nmsg, unsigned int nseg, unsigned int max_msgs,
    unsigned long long max_message_size, /* inflated bytes per message, 0: no limit */
    unsigned int flags,                  /* 0; unknown bits are an error */
    unsigned char* d_dst,
    const unsigned long long* d_dst_off, /* nseg */
    const unsigned long long* d_dst_cap, /* nseg */
    WebsocketInflateMsgRes_t* d_msg_res, /* [s*max_msgs + i] */
    WebsocketInflateResult_t* d_res,     /* nseg */
    void* hip_stream);

/* The inflate list of a batch, from what a reassembly call on the same stream left behind: a pure
 * map, one thread per slot. Slot s*max_frames + i becomes {out_off, len, WEBSOCKET_INFLATE_RAW} when
 * i < min(d_nmsg[s], max_frames), message i is complete, not continued, its first frame's opcode
 * (d_desc[s*max_frames + first_frame].type) is 1 or 2 and that frame's first wire byte
 * (d_buf[d_desc[...].frame_off]) has RSV1 (0x40) set; every other slot of the list becomes
 * {0, 0, WEBSOCKET_INFLATE_SKIP}. The decode calls leave header bytes untouched, so the bit is
 * readable after any of them. out_off is taken as it is (it counts from d_out). With d_out as
 * d_src, and d_nmsg and max_frames reused as d_nmsg and max_msgs, websocketframeBatchInflateDevice
 * then inflates every connection's compressed data messages; the chain is reassemble -> (protocol
 * check with rsv_allowed = 0x40) -> this map -> inflate. Messages still open at the batch end are
 * the caller's: it keeps their parts and submits them with a list of its own once complete.
 * Asynchronous; a NULL pointer, a misaligned array or max_frames == 0 returns a negative code;
 * nseg * max_frames <= 2^30. d_desc and d_msg are 16-B aligned, d_inf_msg 8-B, d_nmsg 4-B. */
WSFRAME_AMD_DEFLATE_EXPORT int websocketframeBatchInflateListFromMessagesDevice(
    const unsigned char* d_buf, const WebsocketFrameDesc_t* d_desc, const WebsocketMsgDesc_t* d_msg,
    const unsigned int* d_nmsg, unsigned int nseg, unsigned int max_frames, WebsocketInflateMsg_t* d_inf_msg,
    void* hip_stream);

/* The same rule for one connection on the host: src[0, src_len) the bodies, msg[0, nmsg) its list,
 * dst[0, dst_cap) its room (out_off counts from dst), msg_res (may be NULL) nmsg records, *out the
 * connection's result. Returns out->out_len, or a negative code for an unknown flag or a NULL
 * required pointer (src only when src_len is 0, msg only when nmsg is 0, dst only when dst_cap is
 * 0), which leaves *out alone. */
WSFRAME_AMD_DEFLATE_EXPORT long long websocketframeInflateHost(
    const unsigned char* src, unsigned long long src_len, const WebsocketInflateMsg_t* msg, unsigned int nmsg,
    unsigned long long max_message_size, unsigned int flags, unsigned char* dst, unsigned long long dst_cap,
    WebsocketInflateMsgRes_t* msg_res, WebsocketInflateResult_t* out);

#ifdef __cplusplus
}
#endif

#endif
