/*
 * wsframe_amd_proto.h — RFC 6455 framing and sequencing check on the device
 * (libwsframe_amd_proto.so: everything libwsframe_amd_text.so exports plus the entry points
 * below, so one library serves a server that decodes, reassembles, validates text and polices
 * the protocol).
 *
 * The decode entry points keep the reference's rule that framing is not judged (RSV ignored,
 * opcode not validated). This check is opt-in and changes nothing in them: it reads the
 * descriptors a decode call just produced and says, per connection, which frame first broke
 * RFC 6455 and which close status to send: 1002 (protocol error) or 1009 (message too big).
 * The text validator's 1007 is the other half of "may I keep this connection?".
 */
#ifndef UTIL_AMD_WSFRAME_AMD_PROTO_H
#define UTIL_AMD_WSFRAME_AMD_PROTO_H

#include "wsframe_amd_text.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Entry points of libwsframe_amd_proto.so only. */
#define WSFRAME_AMD_PROTO_EXPORT __attribute__((visibility("default")))

/* Per-frame codes: the first rule that fails, in this order (0: none). */
enum {
    WEBSOCKET_PROTO_OK = 0,
    WEBSOCKET_PROTO_ERR_RSV = 1,              /* first byte & 0x70 & ~rsv_allowed                        */
    WEBSOCKET_PROTO_ERR_OPCODE = 2,           /* opcode 3..7 or 11..15                                   */
    WEBSOCKET_PROTO_ERR_MASK = 3,             /* EXPECT_MASKED and unmasked, EXPECT_UNMASKED and masked  */
    WEBSOCKET_PROTO_ERR_CTL_FRAGMENTED = 4,   /* control frame (opcode & 8) without FIN                  */
    WEBSOCKET_PROTO_ERR_CTL_LENGTH = 5,       /* control frame with datalen > 125                        */
    WEBSOCKET_PROTO_ERR_CLOSE_LENGTH = 6,     /* CLOSE with datalen 1                                    */
    WEBSOCKET_PROTO_ERR_CLOSE_CODE = 7,       /* CLOSE, datalen >= 2, status code (big-endian u16 of the first
                                                 two body bytes) not in 1000-1003, 1007-1014, 3000-4999;
                                                 1012-1014 are accepted because IANA registered them    */
    WEBSOCKET_PROTO_ERR_CONT_UNEXPECTED = 8,  /* data frame (!(opcode & 8)), opcode 0, no message open   */
    WEBSOCKET_PROTO_ERR_DATA_INTERLEAVED = 9, /* data frame, opcode != 0, a message is open              */
    WEBSOCKET_PROTO_ERR_TOO_BIG = 10,         /* data frame, max_message_size != 0, and the open message's
                                                 bytes before it + datalen > max_message_size            */
    WEBSOCKET_PROTO_AFTER_CLOSE = 0x80,       /* consumed after the connection's first CLOSE: not an error,
                                                 not checked, leaves the state alone                     */
    WEBSOCKET_PROTO_NOT_CONSUMED = 0x81       /* counted in n_frames but not consumed (the frame that stopped
                                                 its segment): not an error, leaves the state alone      */
};

#define WEBSOCKET_PROTO_EXPECT_MASKED   1u  /* a server's rx: every frame must be masked (RFC 6455 5.1)  */
#define WEBSOCKET_PROTO_EXPECT_UNMASKED 2u  /* a client's rx: no frame may be masked                     */
#define WEBSOCKET_PROTO_WIRE_MASKED     4u  /* d_buf still holds masked bodies (after a reassembly call,
                                               which only reads the wire): a masked CLOSE's status code is
                                               XORed with its key, the four bytes before the body. Not
                                               after the in-place decodes, which unmask d_buf             */
#define WEBSOCKET_PROTO_NONE 0xFFFFFFFFu

/* per-connection carry, one u64 per segment, in/out; the caller zeroes it when the connection starts */
#define WEBSOCKET_PROTO_ST_OPEN   (1ULL << 63)  /* a data message is open after the last live data frame */
#define WEBSOCKET_PROTO_ST_CLOSED (1ULL << 62)  /* a CLOSE was consumed                                  */
/* bits 0-55: the open message's bytes so far (sums saturate at 2^56 - 1); 0 whenever OPEN is clear.
   Every other bit is 0. */

/* Per-segment result. 16 bytes. */
typedef struct WebsocketProtoResult_t {
    unsigned int first_bad;    /* least k with an error code 1..10, else WEBSOCKET_PROTO_NONE         */
    unsigned int code;         /* that frame's code, else 0                                           */
    unsigned int close_status; /* 1009 for WEBSOCKET_PROTO_ERR_TOO_BIG, 1002 for the other errors, 0  */
    unsigned int close_frame;  /* the first consumed CLOSE of this batch, else WEBSOCKET_PROTO_NONE   */
} WebsocketProtoResult_t;

/* Check what a decode call (websocketframeBatchDecodeDevice, websocketframeStreamDecodeDevice: one
 * segment at offset 0, or a reassembly call: pass WEBSOCKET_PROTO_WIRE_MASKED) just produced, on the
 * same stream, descriptors at slots s*max_frames. Asynchronous, no host synchronisation; may be
 * captured in a HIP graph after one warm call. nseg == 0 is a no-op. An unknown flag, both EXPECT
 * flags together or rsv_allowed & ~0x70 returns a negative code (websocketframeGpuLastError) and
 * launches nothing.
 *
 * Per segment s, over the counted frames k < d_res[s].n_frames in order:
 *   - frame k is consumed when ret > 0 and frame_off + ret <= d_seg_off[s] + d_res[s].consumed
 *     (64-bit); a counted frame that is not consumed is WEBSOCKET_PROTO_NOT_CONSUMED;
 *   - c = the first consumed frame with type 8 ("before everything" when the incoming state has
 *     CLOSED); consumed frames after c are WEBSOCKET_PROTO_AFTER_CLOSE, c itself is checked;
 *   - the other frames are live. Over the live frames, in error or not: a data frame is one with
 *     !(type & 8); `open` before k is !is_fin of the last live data frame before k, else the
 *     incoming OPEN; `bytes` before k is the datalen sum of the live data frames after the last
 *     live data frame with FIN before k, plus the incoming bytes when there is none;
 *   - a live frame's code is the first rule of the enum above that fails; RSV is read from
 *     d_buf[frame_off], the CLOSE status code from d_buf[data_off], d_buf[data_off + 1];
 *   - state out: OPEN and bytes after the last live data frame (unchanged when there is none),
 *     CLOSED if it was set or c exists. With d_proto_state NULL every batch starts from 0 and
 *     nothing is stored.
 * d_buf is read only at the first header byte of consumed frames and at the two status bytes (plus
 * the four key bytes) of consumed CLOSE frames with 2 <= datalen <= 125; nothing but
 * d_frame_code, d_proto_res, d_proto_state and the library's workspace is written.
 * nseg * max_frames <= 2^30. */
WSFRAME_AMD_PROTO_EXPORT int websocketframeBatchCheckProtocolDevice(
    const unsigned char* d_buf, const unsigned long long* d_seg_off,
    const WebsocketFrameDesc_t* d_desc, const WebsocketSegResult_t* d_res,
    unsigned int nseg, unsigned int max_frames,
    unsigned int flags, unsigned int rsv_allowed, unsigned long long max_message_size,
    unsigned long long* d_proto_state,   /* nseg, in/out, may be NULL                                      */
    unsigned char* d_frame_code,         /* [s*max_frames + k], k < n_frames; optional; other slots never written */
    WebsocketProtoResult_t* d_proto_res, /* nseg                                                           */
    void* hip_stream);

/* The same rule one frame at a time, for connections that stay on the host path: the code of a
 * consumed frame with first header byte b0 (FIN, RSV, opcode), MASK bit `masked` and `datalen`
 * body bytes, of which body2 holds the first two unmasked (read only for a CLOSE with
 * datalen >= 2; may be NULL otherwise); *state is moved past the frame. Invalid flags or
 * rsv_allowed return a negative code and leave *state alone. */
WSFRAME_AMD_PROTO_EXPORT int websocketframeProtoStepHost(unsigned long long* state, unsigned char b0, int masked,
                                                         unsigned long long datalen, const unsigned char body2[2],
                                                         unsigned int flags, unsigned int rsv_allowed,
                                                         unsigned long long max_message_size);

#ifdef __cplusplus
}
#endif

#endif
