/*
 * wsframe_amd_text.h — UTF-8 validation of reassembled text messages on the device
 * (libwsframe_amd_text.so: everything libwsframe_amd_ctl.so exports plus the entry point
 * below, so one library serves a text server).
 *
 * RFC 6455 5.6 / 8.1: a text message (opcode 1) is well-formed UTF-8 over the concatenation of
 * its fragments, and so is a CLOSE reason (5.5.1, 7.1.6); an endpoint that sees otherwise fails
 * the connection with status 1007. The reference never validates: this check is opt-in and
 * changes nothing in the other entry points.
 */
#ifndef UTIL_AMD_WSFRAME_AMD_TEXT_H
#define UTIL_AMD_WSFRAME_AMD_TEXT_H

#include "wsframe_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Entry points of libwsframe_amd_text.so only. */
#define WSFRAME_AMD_TEXT_EXPORT __attribute__((visibility("default")))

enum { WEBSOCKET_TEXT_NA = 0, WEBSOCKET_TEXT_VALID = 1, WEBSOCKET_TEXT_INVALID = 2 };
#define WEBSOCKET_TEXT_NONE 0xFFFFFFFFu

/* per-connection carry, one u32 per segment, in/out; the caller zeroes it when the connection starts */
#define WEBSOCKET_TEXT_ST_PENDING 0x80000000u  /* the message left open is a text message            */
#define WEBSOCKET_TEXT_ST_FAILED  0x40000000u  /* ... and its bytes so far can no longer become valid */
/* bits 24-25: n = 0..3 bytes of an unfinished sequence at the end of the bytes seen so far;
   bits 0-23 : those bytes, first one in bits 0-7. PENDING clear => the word is 0.
   FAILED set => n = 0 and bits 0-23 are 0. */

/* Validate what a reassembly call (websocketframeBatchReassembleDevice, ...Ex or ...Ctl, flags 0
 * or WEBSOCKET_REASM_CONTROL_DIRECT) just produced, on the same stream, descriptors at slots
 * s*max_frames. Asynchronous, no host synchronisation; may be captured in a HIP graph after one
 * warm call. nseg == 0 is a no-op. Returns 0 or a negative code (websocketframeGpuLastError).
 *
 * Per segment s, over messages i < d_nmsg[s] in order; the body of message i is
 * d_out[out_off, out_off + len), its opcode d_desc[s*max_frames + first_frame].type:
 *   - a message with continued == 0 is a text message when its opcode is 1; one with
 *     continued == 1 when the incoming state has PENDING set (d_text_state NULL: it is NA);
 *     a CLOSE (opcode 8, continued 0, complete 1, n_frames 1) is checked over body bytes
 *     [2, len) as a complete string (len < 2: VALID); every other message is WEBSOCKET_TEXT_NA;
 *   - the bytes so far of a text message: the carried unfinished sequence (continued messages)
 *     followed by this batch's body; those of a continued message whose state is FAILED are
 *     hopeless;
 *   - a complete message is VALID when the bytes so far are well-formed UTF-8 (RFC 3629:
 *     shortest form, no surrogates, nothing above U+10FFFF, nothing truncated); an open one when
 *     they are a prefix of a well-formed string (fail-fast, RFC 6455 8.1); else INVALID;
 *   - state out: the last listed message open and text: PENDING, and FAILED or the 0..3 bytes
 *     of its unfinished tail; open and not text: 0; no message open but one continued: 0;
 *     otherwise unchanged (d_nmsg[s] == 0; a control-direct batch of control frames only).
 * Only the 16-B aligned chunks that hold bytes of checked bodies are read, no verdict depends
 * on a byte outside its own body, and nothing but d_verdict, d_first_bad, d_text_state and the
 * library's workspace is written. */
WSFRAME_AMD_TEXT_EXPORT int websocketframeBatchValidateTextDevice(
    const unsigned char* d_out, const WebsocketFrameDesc_t* d_desc,
    const WebsocketMsgDesc_t* d_msg, const unsigned int* d_nmsg,
    unsigned int nseg, unsigned int max_frames,
    unsigned int* d_text_state,   /* nseg, in/out, may be NULL: every batch stands alone          */
    unsigned int* d_verdict,      /* [s*max_frames + i], i < d_nmsg[s]; other slots are not written */
    unsigned int* d_first_bad,    /* nseg, optional: least i with INVALID, else WEBSOCKET_TEXT_NONE */
    void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif
