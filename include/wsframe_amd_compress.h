/*
 * wsframe_amd_compress.h — the send side of RFC 7692 permessage-deflate on the device: every
 * message of a send list is compressed into a room of its own, and a send call that can set RSV1
 * frames the result (libwsframe_amd_pmd.so: everything libwsframe_amd_deflate.so exports plus the
 * entry points below).
 *
 * A compressed message is a raw DEFLATE stream (RFC 1951) that ends with an empty stored block,
 * with that block's last four bytes, 00 00 FF FF, taken off (RFC 7692 section 7.2.1). These calls
 * compress every message on its own, with no window from earlier messages (no context takeover,
 * section 7.1.1), so every message is an independent stream. Opt-in: no other entry point changes.
 *
 * The rule (util_amd/csrc/ws_deflate.h, one definition for the kernel, the host entry point and the
 * CPU test; deterministic: the device writes, byte for byte, what the host entry point writes).
 * Per message of len bytes in a room of cap bytes:
 *   - len == 0 or len < min_len: PLAIN, the body copied to the room unchanged (when it fits);
 *   - else the message is encoded as one fixed-Huffman block (BFINAL 0, BTYPE 01) of LZ77 tokens
 *     (literals; matches of length 4 to 258 at distance 1 to 32,768, never reaching back before the
 *     message's first byte), the end-of-block code and the three header bits 000 of an empty stored
 *     block, zero-padded to the byte: enc_len bytes. Matches come from a hash table of recent
 *     positions, looked up 64 positions at a time and chosen greedily, first position first;
 *   - enc_len < len and enc_len <= cap: DEFLATED, out_len = enc_len;
 *   - else len <= cap: PLAIN, out_len = len (RFC 7692 section 6 allows uncompressed messages: an
 *     incompressible body costs nothing on the wire);
 *   - else WEBSOCKET_DEFLATE_ERR_OUT_SPACE, out_len = 0.
 * A room of max(len, 1) bytes therefore never fails. No dynamic Huffman codes, no stored blocks, no
 * context takeover.
 */
#ifndef UTIL_AMD_WSFRAME_AMD_COMPRESS_H
#define UTIL_AMD_WSFRAME_AMD_COMPRESS_H

#include "wsframe_amd_deflate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Entry points of libwsframe_amd_pmd.so only. */
#define WSFRAME_AMD_PMD_EXPORT __attribute__((visibility("default")))

#define WEBSOCKET_SEND_FLAG_RSV1 1u      /* websocketframeBatchSendExtDevice / SendExtHost: honour WEBSOCKET_SEND_TYPE_RSV1 */
#define WEBSOCKET_SEND_TYPE_RSV1 0x40u   /* WebsocketSendMsg_t.type: the message's first frame carries RSV1 */

/* WebsocketDeflateMsgRes_t.status */
enum {
    WEBSOCKET_DEFLATE_DEFLATED = 0,      /* the room holds the compressed body: send it with RSV1      */
    WEBSOCKET_DEFLATE_PLAIN = 1,         /* the room holds the body unchanged: send it without RSV1    */
    WEBSOCKET_DEFLATE_SKIPPED = 2,       /* a WEBSOCKET_SEND_SKIP entry: nothing read or written        */
    WEBSOCKET_DEFLATE_ERR_OUT_SPACE = 3, /* neither form fits the room                                  */
    WEBSOCKET_DEFLATE_ERR_RANGE = 4      /* src_off + len > src_len (64-bit)                            */
};

/* One message to compress: the layout of WebsocketSendMsg_t, so a send list is a compress list as
 * it stands. type == WEBSOCKET_SEND_SKIP does nothing; any other type is carried along untouched. */
typedef WebsocketSendMsg_t WebsocketDeflateMsg_t;

/* Per-slot result. 24 bytes, 8-B aligned. */
typedef struct WebsocketDeflateMsgRes_t {
    unsigned long long out_off;          /* the slot's room: d_dst_off[s*max_msgs + i] */
    unsigned long long out_len;          /* bytes of the room that hold the message; 0 for SKIPPED and errors */
    unsigned int status;                 /* WEBSOCKET_DEFLATE_* */
    unsigned int reserved;               /* 0 */
} WebsocketDeflateMsgRes_t;

/* Compress the entries d_msg[s*max_msgs + i], i < min(d_nmsg[s], max_msgs), of every connection
 * s < nseg, every entry on its own by the rule above. Asynchronous, no host synchronisation; may be
 * captured in a HIP graph after one warm call. All grids are sized from nseg and max_msgs. An
 * unknown flag (flags is 0), max_msgs == 0, a NULL pointer, a misaligned array or nseg * max_msgs >
 * 2^30 returns a negative code (websocketframeGpuLastError) and launches nothing. nseg == 0 does
 * nothing.
 *
 * Slot q = s*max_msgs + i owns d_dst[d_dst_off[q], d_dst_off[q] + d_dst_cap[q]): its room. No byte
 * outside a slot's room is ever written for it, whatever the verdict; inside the room the bytes
 * past out_len are unspecified. d_msg_res[q] takes out_off = d_dst_off[q], out_len and status:
 *   - type == WEBSOCKET_SEND_SKIP: SKIPPED, out_len 0, nothing is read or written;
 *   - src_off + len > src_len (64-bit): ERR_RANGE, out_len 0;
 *   - else DEFLATED, PLAIN or ERR_OUT_SPACE by the rule above, with min_len as given (0: compress
 *     every message that has a byte).
 * Slots at or past min(d_nmsg[s], max_msgs) are not written. Nothing but the rooms and d_msg_res is
 * written (the call needs no workspace); d_src is read only inside the ranges of entries that run.
 * The rooms overlap neither each other nor d_src. d_msg, d_dst_off, d_dst_cap and d_msg_res are 8-B
 * aligned, d_nmsg 4-B; d_src and d_dst may lie anywhere. One wavefront compresses one message. */
WSFRAME_AMD_PMD_EXPORT int websocketframeBatchDeflateDevice(
    const unsigned char* d_src, unsigned long long src_len,
    const WebsocketDeflateMsg_t* d_msg,  /* [s*max_msgs + i], i < d_nmsg[s] */
    const unsigned int* d_nmsg, unsigned int nseg, unsigned int max_msgs,
    unsigned long long min_len,          /* shorter messages are not compressed */
    unsigned int flags,                  /* 0; unknown bits are an error */
    unsigned char* d_dst,
    const unsigned long long* d_dst_off, /* [s*max_msgs + i] */
    const unsigned long long* d_dst_cap, /* [s*max_msgs + i] */
    WebsocketDeflateMsgRes_t* d_msg_res, /* [s*max_msgs + i] */
    void* hip_stream);

/* The send list of what a deflate call on the same stream left behind: a pure map, one thread per
 * slot. Slot s*max_msgs + i, i < min(d_nmsg[s], max_msgs), becomes {out_off, out_len, type |
 * WEBSOCKET_SEND_TYPE_RSV1} for a DEFLATED result, {out_off, out_len, type} for a PLAIN one (type:
 * d_msg's) and {0, 0, WEBSOCKET_SEND_SKIP} for everything else. With d_dst as d_src,
 * websocketframeBatchSendExtDevice with WEBSOCKET_SEND_FLAG_RSV1 then sends every message in its
 * shorter form. Slots at or past d_nmsg[s] are not written. Asynchronous; a NULL pointer, a
 * misaligned array or max_msgs == 0 returns a negative code; nseg * max_msgs <= 2^30. d_msg,
 * d_msg_res and d_send_msg are 8-B aligned, d_nmsg 4-B. */
WSFRAME_AMD_PMD_EXPORT int websocketframeBatchSendListFromDeflatedDevice(
    const WebsocketDeflateMsg_t* d_msg, const unsigned int* d_nmsg, unsigned int nseg, unsigned int max_msgs,
    const WebsocketDeflateMsgRes_t* d_msg_res, WebsocketSendMsg_t* d_send_msg, void* hip_stream);

/* websocketframeBatchSendDevice (wsframe_amd_send.h: same arguments, results and contract) that
 * also accepts flags == WEBSOCKET_SEND_FLAG_RSV1. Under that flag an entry whose type has
 * WEBSOCKET_SEND_TYPE_RSV1 set carries RSV1 on its first frame and only there (RFC 7692 section
 * 6.1): continuation frames never do. The opcode is type & 0x0F as before. With flags == 0 it is
 * websocketframeBatchSendDevice. */
WSFRAME_AMD_PMD_EXPORT int websocketframeBatchSendExtDevice(
    const unsigned char* d_src, unsigned long long src_len, const WebsocketSendMsg_t* d_msg,
    const unsigned int* d_nmsg, unsigned int nseg, unsigned int max_msgs, const unsigned int* d_frag_size,
    const unsigned int* d_mask_key, unsigned int flags, unsigned char* d_tx, unsigned long long tx_capacity,
    unsigned long long* d_tx_off, unsigned long long* d_msg_tx_off, WebsocketSendResult_t* d_send_res,
    void* hip_stream);

/* The deflate rule for one connection's list on the host: src[0, src_len) the bodies, msg[0, nmsg)
 * the list, dst the base of the rooms, dst_off / dst_cap / msg_res nmsg entries each. Returns the
 * number of entries that ended DEFLATED or PLAIN, or a negative code for an unknown flag or a NULL
 * required pointer (src only when src_len is 0; msg, dst_off, dst_cap and msg_res only when nmsg is
 * 0; dst never checked: a list of empty rooms needs none), which writes nothing. */
WSFRAME_AMD_PMD_EXPORT long long websocketframeDeflateHost(
    const unsigned char* src, unsigned long long src_len, const WebsocketDeflateMsg_t* msg, unsigned int nmsg,
    unsigned long long min_len, unsigned int flags, unsigned char* dst, const unsigned long long* dst_off,
    const unsigned long long* dst_cap, WebsocketDeflateMsgRes_t* msg_res);

/* websocketframeSendHost (wsframe_amd_send.h) that also accepts flags == WEBSOCKET_SEND_FLAG_RSV1,
 * with the meaning it has in websocketframeBatchSendExtDevice. */
WSFRAME_AMD_PMD_EXPORT long long websocketframeSendExtHost(
    const unsigned char* src, unsigned long long src_len, const WebsocketSendMsg_t* msg, unsigned int nmsg,
    unsigned int frag_size, const unsigned int* mask_key, unsigned int flags, unsigned char* tx,
    unsigned long long tx_capacity, unsigned long long* msg_tx_off, WebsocketSendResult_t* out);

#ifdef __cplusplus
}
#endif

#endif
