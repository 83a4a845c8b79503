"""Python mirror of the websocketframe API (inc/crt/protocol/websocketframe.h:10-49)
and of the batch API (include/wsframe_amd.h Part 2), over libwsframe_amd.so.

Host functions take a mutable ``bytearray``/numpy uint8 buffer and behave like
the C functions (same argument meaning, same return conventions: >0 bytes
consumed, 0 incomplete, <0 error). Batch functions take torch CUDA tensors and
only pass raw device pointers and the current HIP stream to the C ABI.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import WsDesc, WsSegRes, check, check_bench, load_bench_lib, load_ctl_lib, load_lib

WEBSOCKET_CONTINUE_FRAME = 0
WEBSOCKET_TEXT_FRAME = 1
WEBSOCKET_BINARY_FRAME = 2
WEBSOCKET_CLOSE_FRAME = 8
WEBSOCKET_PING_FRAME = 9
WEBSOCKET_PONG_FRAME = 10
WEBSOCKET_MAX_ENCODE_HEADLENGTH = 10

SEG_OK, SEG_MAX_FRAMES, SEG_ERR_DECODE, SEG_ERR_LEN_WRAP = 0, 1, -1, -2
SEG_ERR_OUT_SPACE = -3
SEG_ERR_CACHE_OVERFLOW = -4
REASM_CONTROL_DIRECT = 1  # WEBSOCKET_REASM_CONTROL_DIRECT: control frames delivered apart from fragmented messages
# include/wsframe_amd_text.h: verdicts of batch_validate_text_device, its "no INVALID message" value and state bits
TEXT_NA, TEXT_VALID, TEXT_INVALID = 0, 1, 2
TEXT_NONE = 0xFFFFFFFF
TEXT_ST_PENDING, TEXT_ST_FAILED = 0x80000000, 0x40000000
# the validator's geometry (ws_utf8.hip): 16-B chunk per lane, 64 chunks per wave row, 4 rows per tile
TEXT_CHUNK, TEXT_ROW, TEXT_TILE = 16, 1024, 4096
# include/wsframe_amd_proto.h: frame codes of batch_check_protocol_device, its flags and state bits
(PROTO_OK, PROTO_ERR_RSV, PROTO_ERR_OPCODE, PROTO_ERR_MASK, PROTO_ERR_CTL_FRAGMENTED, PROTO_ERR_CTL_LENGTH,
 PROTO_ERR_CLOSE_LENGTH, PROTO_ERR_CLOSE_CODE, PROTO_ERR_CONT_UNEXPECTED, PROTO_ERR_DATA_INTERLEAVED,
 PROTO_ERR_TOO_BIG) = range(11)
PROTO_AFTER_CLOSE, PROTO_NOT_CONSUMED = 0x80, 0x81
PROTO_EXPECT_MASKED, PROTO_EXPECT_UNMASKED, PROTO_WIRE_MASKED = 1, 2, 4
PROTO_NONE = 0xFFFFFFFF
PROTO_ST_OPEN, PROTO_ST_CLOSED, PROTO_BYTES_MAX = 1 << 63, 1 << 62, (1 << 56) - 1
NETPACKET_FRAGMENT = 6  # transport_ctx.h:11-18; the pktype websocketframeOnDecode reports
DATA_OFF_NULL = 0xFFFFFFFFFFFFFFFF
BATCH_PAD = 32  # WEBSOCKET_BATCH_PAD: readable device bytes required after every segment

DESC_DTYPE = np.dtype([("frame_off", "<u8"), ("data_off", "<u8"), ("datalen", "<u8"), ("ret", "<i4"),
                       ("is_fin", "u1"), ("type", "u1"), ("masked", "u1"), ("hdrlen", "u1")])
SEGRES_DTYPE = np.dtype([("consumed", "<u8"), ("n_frames", "<u4"), ("status", "<i4")])
MSG_DTYPE = np.dtype([("out_off", "<u8"), ("len", "<u8"), ("first_frame", "<u4"), ("n_frames", "<u4"),
                      ("complete", "<u4"), ("continued", "<u4")])
assert MSG_DTYPE.itemsize == 32
ENC_DTYPE = np.dtype([("src_off", "<u8"), ("len", "<u8"), ("mask_key", "<u4"), ("type", "u1"), ("is_fin", "u1"),
                      ("prev_is_fin", "u1"), ("masked", "u1")])
assert ENC_DTYPE.itemsize == 24
PROTO_RES_DTYPE = np.dtype([("first_bad", "<u4"), ("code", "<u4"), ("close_status", "<u4"), ("close_frame", "<u4")])
assert PROTO_RES_DTYPE.itemsize == 16
# include/wsframe_amd_handshake.h: the descriptor of batch_handshake_device / handshake_host, its flags, the call flag
HS_DTYPE = np.dtype([("ret", "<i4"), ("key_off", "<u4"), ("key_len", "<u4"), ("proto_off", "<u4"), ("proto_len", "<u4"),
                     ("resp_len", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
assert HS_DTYPE.itemsize == 32
HS_NONE = 0xFFFFFFFF
HS_RESP_WRITTEN, HS_RESP_NO_SPACE, HS_ERR_SEG_LEN = 1, 2, 4
HS_ECHO_PROTOCOL = 1
# include/wsframe_amd_reply.h: the result of batch_control_replies_device / control_replies_host, close kinds, flags, state
REPLY_RES_DTYPE = np.dtype([("n_pong", "<u4"), ("close_kind", "<u4"), ("close_status", "<u4"), ("tx_len", "<u4")])
assert REPLY_RES_DTYPE.itemsize == 16
REPLY_CLOSE_NONE, REPLY_CLOSE_ECHO, REPLY_CLOSE_PROTOCOL, REPLY_CLOSE_CALLER = range(4)
REPLY_WIRE_MASKED, REPLY_LAST_PING_ONLY = 4, 8
REPLY_ST_CLOSE_SENT = 1
REPLY_NONE = 0xFFFFFFFF
# include/wsframe_amd_send.h: the message entry and the result of batch_send_device / send_host, its status values
SEND_MSG_DTYPE = np.dtype([("src_off", "<u8"), ("len", "<u8"), ("type", "<u4"), ("reserved", "<u4")])
assert SEND_MSG_DTYPE.itemsize == 24
SEND_RES_DTYPE = np.dtype([("tx_len", "<u8"), ("n_frames", "<u8"), ("n_msgs", "<u4"), ("status", "<u4"),
                           ("first_bad", "<u4"), ("reserved", "<u4")])
assert SEND_RES_DTYPE.itemsize == 32
SEND_SKIP = SEND_NONE = SEND_FRAG_DEFAULT = 0xFFFFFFFF
SEND_OK, SEND_ERR_FRAGMENT_SIZE, SEND_ERR_RANGE = range(3)
# include/wsframe_amd_deflate.h: the entry and the two results of batch_inflate_device / inflate_host, kinds, status values
INFLATE_MSG_DTYPE = np.dtype([("src_off", "<u8"), ("len", "<u8"), ("kind", "<u4"), ("reserved", "<u4")])
INFLATE_MSGRES_DTYPE = np.dtype([("out_off", "<u8"), ("out_len", "<u8"), ("status", "<u4"), ("reserved", "<u4")])
INFLATE_RES_DTYPE = np.dtype([("out_len", "<u8"), ("n_msgs", "<u4"), ("status", "<u4"), ("first_bad", "<u4"),
                              ("close_status", "<u4")])
assert INFLATE_MSG_DTYPE.itemsize == INFLATE_MSGRES_DTYPE.itemsize == INFLATE_RES_DTYPE.itemsize == 24
INFLATE_SKIP = INFLATE_NONE = 0xFFFFFFFF
INFLATE_RAW = 1
# include/wsframe_amd_compress.h (libwsframe_amd_pmd.so): a compress list is a send list (SEND_MSG_DTYPE)
DEFLATE_MSG_DTYPE = SEND_MSG_DTYPE
DEFLATE_MSGRES_DTYPE = np.dtype([("out_off", "<u8"), ("out_len", "<u8"), ("status", "<u4"), ("reserved", "<u4")])
(DEFLATE_DEFLATED, DEFLATE_PLAIN, DEFLATE_SKIPPED, DEFLATE_ERR_OUT_SPACE, DEFLATE_ERR_RANGE) = range(5)
SEND_FLAG_RSV1 = 1
SEND_TYPE_RSV1 = 0x40
(INFLATE_OK, INFLATE_ERR_DATA, INFLATE_ERR_TOO_BIG, INFLATE_ERR_OUT_SPACE, INFLATE_ERR_RANGE,
 INFLATE_NOT_RUN) = range(6)
# include/wsframe_amd_client.h: the entry, the two descriptors, the flags and the reasons of the client handshake
CLI_ENTRY_DTYPE = np.dtype([("path_off", "<u8"), ("proto_off", "<u8"), ("host_off", "<u8"), ("path_len", "<u4"),
                            ("proto_len", "<u4"), ("host_len", "<u4"), ("reserved", "<u4", (3,))])
assert CLI_ENTRY_DTYPE.itemsize == 48
CLI_REQ_DTYPE = np.dtype([("req_len", "<u4"), ("key_off", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
assert CLI_REQ_DTYPE.itemsize == 16
CLI_VERIFY_DTYPE = np.dtype([("ret", "<i4"), ("reason", "<u4"), ("status", "<u4"), ("proto_off", "<u4"), ("proto_len", "<u4"),
                             ("accept_off", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
assert CLI_VERIFY_DTYPE.itemsize == 32
CLI_NONE = 0xFFFFFFFF
CLI_REQ_WRITTEN, CLI_REQ_NO_SPACE, CLI_ERR_RANGE, CLI_ERR_BYTES, CLI_ERR_SEG_LEN = 1, 2, 4, 8, 16
(CLI_OK, CLI_REASON_STATUS, CLI_REASON_UPGRADE, CLI_REASON_CONNECTION, CLI_REASON_ACCEPT, CLI_REASON_EXTENSION,
 CLI_REASON_PROTOCOL, CLI_REASON_TOO_LONG) = range(8)
assert DESC_DTYPE.itemsize == C.sizeof(WsDesc) == 32
assert SEGRES_DTYPE.itemsize == C.sizeof(WsSegRes) == 16


def _addr(buf):
    """address of a writable host buffer (bytearray or numpy array)"""
    if isinstance(buf, np.ndarray):
        return buf.ctypes.data
    return C.addressof((C.c_char * len(buf)).from_buffer(buf))


# ------------------------------------------------------------------ host, one frame

def websocketframeDecode(buf, length=None, offset=0):
    """websocketframe.c:112-165 on buf[offset:offset+length], in place.

    Returns (ret, data_off, datalen, is_fin, type); data_off is the payload offset
    into ``buf`` (None where the C function sets *data = NULL). Out-params the C
    function leaves untouched (ret 0) come back as None.
    """
    lib = load_lib()
    if length is None:
        length = len(buf) - offset
    sent = 0xA5A5A5A5A5A5A5A5
    data, datalen, fin, typ = C.c_void_p(sent), C.c_ulonglong(sent), C.c_int(-7), C.c_int(-7)
    base = _addr(buf) if len(buf) else 0
    r = lib.websocketframeDecode(base + offset, length, C.byref(data), C.byref(datalen), C.byref(fin), C.byref(typ))
    if data.value == sent:
        return r, None, None, None, None
    doff = None if data.value is None else data.value - base
    return r, doff, datalen.value, fin.value, typ.value


def websocketframeEncodeHeadLength(datalen):
    return load_lib().websocketframeEncodeHeadLength(datalen)


def websocketframeEncode(is_fin, prev_is_fin, type_, datalen):
    """websocketframe.c:176-202; returns the header bytes"""
    lib = load_lib()
    h = (C.c_ubyte * WEBSOCKET_MAX_ENCODE_HEADLENGTH)()
    lib.websocketframeEncode(h, is_fin, prev_is_fin, type_, datalen)
    return bytes(h)[: lib.websocketframeEncodeHeadLength(datalen)]


def websocketframeComputeSecAccept(sec_key):
    lib = load_lib()
    out = C.create_string_buffer(60)
    r = lib.websocketframeComputeSecAccept(sec_key, len(sec_key), out)
    return out.value.decode() if r else None


def websocketframeDecodeHandshakeRequest(data):
    """returns (ret, sec_key_off, sec_key_len, sec_protocol_off, sec_protocol_len); offsets
    into ``data`` or None (NULL) / "untouched" when the C function does not write them"""
    lib = load_lib()
    buf = C.create_string_buffer(bytes(data), len(data))
    sent = 0xA5A5A5A5A5A5A5A5
    sk, skl, sp, spl = C.c_void_p(sent), C.c_uint(777), C.c_void_p(sent), C.c_uint(777)
    r = lib.websocketframeDecodeHandshakeRequest(buf, len(data), C.byref(sk), C.byref(skl), C.byref(sp), C.byref(spl))
    base = C.addressof(buf)

    def off(p):
        return "untouched" if p.value == sent else (None if p.value is None else p.value - base)
    return r, off(sk), skl.value, off(sp), spl.value


def websocketframeEncodeHandshakeResponse(sec_accept):
    lib = load_lib()
    out = C.create_string_buffer(162)
    return C.string_at(lib.websocketframeEncodeHandshakeResponse(sec_accept, len(sec_accept), out)).decode()


def websocketframeEncodeHandshakeResponseWithProtocol(sec_accept, sec_protocol):
    lib = load_lib()
    p = lib.websocketframeEncodeHandshakeResponseWithProtocol(
        sec_accept, len(sec_accept), sec_protocol, len(sec_protocol) if sec_protocol else 0)
    if not p:
        return None
    s = C.string_at(p).decode()
    lib.websocketframeFreeString(p)
    return s


# ------------------------------------------------------------------ batch, device

def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(stream):
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream


def batch_decode_device(buf, seg_off, seg_len, max_frames, desc, res, desc_base=None, stream=None):
    """websocketframeBatchDecodeDevice on torch CUDA tensors (uint8 buf, int64 seg_off/
    seg_len/desc_base, desc: uint8 [>= 32*slots], res: uint8 [16*nseg]); async on `stream`."""
    nseg = seg_off.numel()
    assert buf.numel() >= BATCH_PAD, "device batch needs WEBSOCKET_BATCH_PAD bytes of slack"
    assert seg_len.numel() == nseg and res.numel() * res.element_size() >= 16 * nseg
    if desc_base is None:
        assert desc.numel() * desc.element_size() >= 32 * nseg * max_frames, "desc holds < nseg*max_frames slots"
    assert buf.is_cuda and seg_off.is_cuda and seg_len.is_cuda and desc.is_cuda and res.is_cuda
    # buflen: segments lie in [0, numel - PAD); the last PAD bytes are the readable slack
    rc = load_lib().websocketframeBatchDecodeDevice(_ptr(buf), buf.numel() - BATCH_PAD, _ptr(seg_off), _ptr(seg_len),
                                                    nseg, max_frames, _ptr(desc_base), _ptr(desc), _ptr(res),
                                                    _stream(stream))
    check(rc, "websocketframeBatchDecodeDevice")


def stream_decode_device(buf, length, max_frames, desc, res, stream=None):
    """websocketframeStreamDecodeDevice: one raw stream buf[0:length) (uint8 CUDA tensor with
    >= BATCH_PAD bytes after it), decoded in place; asynchronous on `stream` (graph-capturable;
    an eager call on a stream of >= 512 KiB reads the pass state back)."""
    assert buf.numel() >= length + BATCH_PAD
    rc = load_lib().websocketframeStreamDecodeDevice(_ptr(buf), length, max_frames, _ptr(desc), _ptr(res),
                                                     _stream(stream))
    check(rc, "websocketframeStreamDecodeDevice")


def batch_reassemble_device(buf, seg_off, seg_len, max_frames, desc, res, out, msg, nmsg, out_off=None, open_state=None,
                            stream=None, readcache_max=0, cached=None, flags=0):
    """websocketframeBatchReassembleDeviceEx on torch CUDA tensors: buf (uint8, wire, read only;
    the last BATCH_PAD bytes are slack), seg_off/seg_len/out_off (int64), desc (uint8
    >= 32*nseg*max_frames), res (uint8 16*nseg), out (uint8), msg (uint8 >= 32*nseg*max_frames),
    nmsg (int32 nseg), open_state (uint8 nseg, in/out, optional), readcache_max (the channel's
    readcache_max_size, 0 = unlimited), cached (int32 nseg, in/out, optional: the pending
    message's cached bytes, u32); async on `stream`. flags: 0, or REASM_CONTROL_DIRECT
    (websocketframeBatchReassembleDeviceCtl of libwsframe_amd_ctl.so: every control frame is a message of its own, its
    body packed downward from its region's end)."""
    nseg = seg_off.numel()
    assert buf.numel() >= BATCH_PAD and seg_len.numel() == nseg and nmsg.numel() >= nseg
    assert desc.numel() * desc.element_size() >= 32 * nseg * max_frames
    assert msg.numel() * msg.element_size() >= 32 * nseg * max_frames
    assert res.numel() * res.element_size() >= 16 * nseg
    assert cached is None or cached.numel() * cached.element_size() >= 4 * nseg
    if flags:
        rc = load_ctl_lib().websocketframeBatchReassembleDeviceCtl(
            _ptr(buf), buf.numel() - BATCH_PAD, _ptr(seg_off), _ptr(seg_len), nseg, max_frames, _ptr(desc), _ptr(res),
            _ptr(out), _ptr(out_off), _ptr(msg), _ptr(nmsg), _ptr(open_state), int(readcache_max), _ptr(cached),
            int(flags), _stream(stream))
        check(rc, "websocketframeBatchReassembleDeviceCtl", load_ctl_lib())
        return
    rc = load_lib().websocketframeBatchReassembleDeviceEx(
        _ptr(buf), buf.numel() - BATCH_PAD, _ptr(seg_off), _ptr(seg_len), nseg, max_frames, _ptr(desc), _ptr(res),
        _ptr(out), _ptr(out_off), _ptr(msg), _ptr(nmsg), _ptr(open_state), int(readcache_max), _ptr(cached),
        _stream(stream))
    check(rc, "websocketframeBatchReassembleDeviceEx")


def batch_validate_text_device(out, desc, msg, nmsg, max_frames, verdict, text_state=None, first_bad=None, stream=None):
    """websocketframeBatchValidateTextDevice (libwsframe_amd_text.so) on what a reassembly call on
    the same stream just produced: out (uint8), desc / msg (uint8 >= 32*nseg*max_frames), nmsg
    (int32 nseg); verdict (int32 >= nseg*max_frames: TEXT_NA / TEXT_VALID / TEXT_INVALID at slot
    s*max_frames + i, i < nmsg[s]; other slots are not written), text_state (int32 nseg, in/out,
    optional: the per-connection carry, zero when the connection starts), first_bad (int32 nseg,
    optional: the least i with TEXT_INVALID, else TEXT_NONE as u32); async on `stream`."""
    nseg = nmsg.numel()
    assert desc.numel() * desc.element_size() >= 32 * nseg * max_frames
    assert msg.numel() * msg.element_size() >= 32 * nseg * max_frames
    assert verdict.numel() * verdict.element_size() >= 4 * nseg * max_frames
    assert text_state is None or text_state.numel() * text_state.element_size() >= 4 * nseg
    assert first_bad is None or first_bad.numel() * first_bad.element_size() >= 4 * nseg
    lib = _lib.load_text_lib()
    rc = lib.websocketframeBatchValidateTextDevice(_ptr(out), _ptr(desc), _ptr(msg), _ptr(nmsg), nseg, max_frames,
                                                   _ptr(text_state), _ptr(verdict), _ptr(first_bad), _stream(stream))
    check(rc, "websocketframeBatchValidateTextDevice", lib)


def batch_check_protocol_device(buf, seg_off, desc, res, max_frames, proto_res, flags=0, rsv_allowed=0,
                                max_message_size=0, proto_state=None, frame_code=None, stream=None):
    """websocketframeBatchCheckProtocolDevice (libwsframe_amd_proto.so) on what a decode or reassembly
    call on the same stream just produced: buf (uint8, the wire), seg_off (int64 nseg), desc (uint8
    >= 32*nseg*max_frames), res (uint8 16*nseg); proto_res (uint8 16*nseg: PROTO_RES_DTYPE records),
    proto_state (int64 nseg, in/out, optional: the per-connection carry, zero when the connection
    starts), frame_code (uint8 >= nseg*max_frames, optional: the code of frame k of segment s at
    s*max_frames + k, k < n_frames; other slots are not written). flags: PROTO_EXPECT_MASKED or
    PROTO_EXPECT_UNMASKED, and PROTO_WIRE_MASKED after a reassembly call; async on `stream`."""
    nseg = seg_off.numel()
    assert desc.numel() * desc.element_size() >= 32 * nseg * max_frames
    assert res.numel() * res.element_size() >= 16 * nseg
    assert proto_res.numel() * proto_res.element_size() >= 16 * nseg
    assert proto_state is None or proto_state.numel() * proto_state.element_size() >= 8 * nseg
    assert frame_code is None or frame_code.numel() * frame_code.element_size() >= nseg * max_frames
    lib = _lib.load_proto_lib()
    rc = lib.websocketframeBatchCheckProtocolDevice(_ptr(buf), _ptr(seg_off), _ptr(desc), _ptr(res), nseg, max_frames,
                                                    int(flags), int(rsv_allowed), int(max_message_size),
                                                    _ptr(proto_state), _ptr(frame_code), _ptr(proto_res), _stream(stream))
    check(rc, "websocketframeBatchCheckProtocolDevice", lib)


def proto_step_host(state, b0, masked, datalen, body2=None, flags=0, rsv_allowed=0, max_message_size=0):
    """websocketframeProtoStepHost: (code, new state) of one consumed frame on the host path"""
    st = C.c_ulonglong(state)
    code = _lib.load_proto_lib().websocketframeProtoStepHost(C.byref(st), b0, int(masked), datalen, body2, flags,
                                                             rsv_allowed, max_message_size)
    return code, st.value


def batch_control_replies_device(buf, seg_off, desc, res, max_frames, tx, tx_off, reply_res, flags=0, proto_res=None,
                                 fail_status=None, mask_key=None, reply_state=None, tx_capacity=None, stream=None):
    """websocketframeBatchControlRepliesDevice (libwsframe_amd_reply.so) on what a decode call and,
    optionally, batch_check_protocol_device on the same stream just produced: buf (uint8, the wire),
    seg_off (int64 nseg), desc (uint8 >= 32*nseg*max_frames), res (uint8 16*nseg); tx (uint8: the
    reply bytes; 131 B per counted frame + 8 B per segment always suffice), tx_off (int64 nseg + 1:
    segment s's reply is tx[tx_off[s]:tx_off[s+1]]), reply_res (uint8 16*nseg: REPLY_RES_DTYPE
    records); proto_res (uint8 16*nseg, optional), fail_status (int32 nseg, optional), mask_key
    (int32 nseg*(max_frames+1), optional: client role), reply_state (int32 nseg, in/out, optional:
    the per-connection carry, zero when the connection starts). flags: REPLY_WIRE_MASKED after a
    reassembly call, REPLY_LAST_PING_ONLY; tx_capacity defaults to tx.numel(); async on `stream`."""
    nseg = seg_off.numel()
    assert desc.numel() * desc.element_size() >= 32 * nseg * max_frames
    assert res.numel() * res.element_size() >= 16 * nseg
    assert reply_res.numel() * reply_res.element_size() >= 16 * nseg
    assert tx_off.numel() * tx_off.element_size() >= 8 * (nseg + 1)
    assert proto_res is None or proto_res.numel() * proto_res.element_size() >= 16 * nseg
    assert fail_status is None or fail_status.numel() * fail_status.element_size() >= 4 * nseg
    assert mask_key is None or mask_key.numel() * mask_key.element_size() >= 4 * nseg * (max_frames + 1)
    assert reply_state is None or reply_state.numel() * reply_state.element_size() >= 4 * nseg
    cap = (0 if tx is None else tx.numel()) if tx_capacity is None else tx_capacity
    lib = _lib.load_reply_lib()
    rc = lib.websocketframeBatchControlRepliesDevice(_ptr(buf), _ptr(seg_off), _ptr(desc), _ptr(res), nseg, max_frames,
                                                     int(flags), _ptr(proto_res), _ptr(fail_status), _ptr(mask_key),
                                                     _ptr(reply_state), _ptr(tx), int(cap), _ptr(tx_off), _ptr(reply_res),
                                                     _stream(stream))
    check(rc, "websocketframeBatchControlRepliesDevice", lib)


def control_replies_host(buf, seg_off, desc, res, max_frames, flags=0, proto_res=None, fail_status=0, mask_key=None,
                         state=0, tx_capacity=None):
    """websocketframeControlRepliesHost on one segment: buf (numpy uint8), desc (DESC_DTYPE, the
    segment's max_frames slots), res (one SEGRES_DTYPE record), proto_res (one PROTO_RES_DTYPE record
    or None), mask_key (numpy uint32, max_frames + 1, or None), state (the carry in, or None: no
    carry). Returns (reply length, the reply bytes that fit in tx_capacity, REPLY_RES_DTYPE record,
    state out)."""
    lib = _lib.load_reply_lib()
    desc = np.ascontiguousarray(desc)
    res = np.ascontiguousarray(res).reshape(1)
    pr = None if proto_res is None else np.ascontiguousarray(proto_res).reshape(1)
    keys = None if mask_key is None else np.ascontiguousarray(mask_key, dtype=np.uint32)
    cap = 131 * max_frames + 8 if tx_capacity is None else tx_capacity
    tx = np.zeros(max(1, cap), np.uint8)
    out = np.zeros(1, REPLY_RES_DTYPE)
    st = None if state is None else C.c_uint(state)
    n = lib.websocketframeControlRepliesHost(buf.ctypes.data, int(seg_off), desc.ctypes.data, res.ctypes.data, max_frames,
                                             int(flags), None if pr is None else pr.ctypes.data, int(fail_status),
                                             None if keys is None else keys.ctypes.data,
                                             None if st is None else C.addressof(st), tx.ctypes.data, cap, out.ctypes.data)
    if n < 0:
        check(-1, "websocketframeControlRepliesHost", lib)
    return n, bytes(tx[:min(n, cap)]), out[0], None if st is None else st.value


def batch_send_device(src, msg, nmsg, max_msgs, tx, tx_off, send_res, frag_size=None, mask_key=None, msg_tx_off=None,
                      tx_capacity=None, src_len=None, flags=0, stream=None):
    """websocketframeBatchSendDevice (libwsframe_amd_send.so) on torch CUDA tensors: src (uint8, the
    bodies), msg (uint8 >= 24*nseg*max_msgs: SEND_MSG_DTYPE records at s*max_msgs + i), nmsg (int32
    nseg), frag_size (int32 nseg, optional: every connection's write_fragment_size), mask_key (int32
    nseg*max_msgs, optional: client role); tx (uint8: the wire bytes; None with tx_capacity 0 sizes),
    tx_off (int64 nseg + 1: connection s owns tx[tx_off[s]:tx_off[s+1]]), msg_tx_off (int64
    nseg*max_msgs, optional), send_res (uint8 32*nseg: SEND_RES_DTYPE records). tx_capacity defaults
    to tx.numel(), src_len to src.numel(); async on `stream`."""
    nseg = nmsg.numel()
    assert msg.numel() * msg.element_size() >= 24 * nseg * max_msgs
    assert tx_off.numel() * tx_off.element_size() >= 8 * (nseg + 1)
    assert send_res.numel() * send_res.element_size() >= 32 * nseg
    assert frag_size is None or frag_size.numel() * frag_size.element_size() >= 4 * nseg
    assert mask_key is None or mask_key.numel() * mask_key.element_size() >= 4 * nseg * max_msgs
    assert msg_tx_off is None or msg_tx_off.numel() * msg_tx_off.element_size() >= 8 * nseg * max_msgs
    cap = (0 if tx is None else tx.numel()) if tx_capacity is None else tx_capacity
    lib = _lib.load_send_lib()
    rc = lib.websocketframeBatchSendDevice(_ptr(src), int(src.numel() if src_len is None else src_len), _ptr(msg), _ptr(nmsg),
                                           nseg, int(max_msgs), _ptr(frag_size), _ptr(mask_key), int(flags), _ptr(tx),
                                           int(cap), _ptr(tx_off), _ptr(msg_tx_off), _ptr(send_res), _stream(stream))
    check(rc, "websocketframeBatchSendDevice", lib)


def batch_send_list_from_messages_device(desc, msg, nmsg, max_frames, send_msg, stream=None):
    """websocketframeBatchSendListFromMessagesDevice: the echo's send list (uint8 >= 24*nseg*max_frames)
    from what batch_reassemble_device left in desc, msg and nmsg; async on `stream`."""
    nseg = nmsg.numel()
    assert desc.numel() * desc.element_size() >= 32 * nseg * max_frames
    assert msg.numel() * msg.element_size() >= 32 * nseg * max_frames
    assert send_msg.numel() * send_msg.element_size() >= 24 * nseg * max_frames
    lib = _lib.load_send_lib()
    rc = lib.websocketframeBatchSendListFromMessagesDevice(_ptr(desc), _ptr(msg), _ptr(nmsg), nseg, int(max_frames),
                                                           _ptr(send_msg), _stream(stream))
    check(rc, "websocketframeBatchSendListFromMessagesDevice", lib)


def send_host(src, msg, frag_size=SEND_FRAG_DEFAULT, mask_key=None, tx_capacity=None, flags=0):
    """websocketframeSendHost on one connection: src (numpy uint8), msg (SEND_MSG_DTYPE array),
    mask_key (numpy uint32, one per message, or None). Returns (full length, the wire bytes that
    fit in tx_capacity, every message's offset, SEND_RES_DTYPE record)."""
    lib = _lib.load_send_lib()
    src = np.ascontiguousarray(src, dtype=np.uint8)
    msg = np.ascontiguousarray(msg, dtype=SEND_MSG_DTYPE)
    keys = None if mask_key is None else np.ascontiguousarray(mask_key, dtype=np.uint32)
    out = np.zeros(1, SEND_RES_DTYPE)
    moff = np.zeros(max(1, len(msg)), np.uint64)
    pad = np.zeros(1, np.uint8)
    sp = src.ctypes.data if len(src) else pad.ctypes.data
    if tx_capacity is None:
        tx_capacity = lib.websocketframeSendHost(sp, len(src), msg.ctypes.data, len(msg), int(frag_size),
                                                 None if keys is None else keys.ctypes.data, int(flags), None, 0, None,
                                                 out.ctypes.data)
        if tx_capacity < 0:
            check(-1, "websocketframeSendHost", lib)
    tx = np.zeros(max(1, tx_capacity), np.uint8)
    n = lib.websocketframeSendHost(sp, len(src), msg.ctypes.data, len(msg), int(frag_size),
                                   None if keys is None else keys.ctypes.data, int(flags), tx.ctypes.data, tx_capacity,
                                   moff.ctypes.data, out.ctypes.data)
    if n < 0:
        check(-1, "websocketframeSendHost", lib)
    return n, bytes(tx[:min(n, tx_capacity)]), moff[:len(msg)], out[0]


def batch_inflate_device(src, msg, nmsg, max_msgs, dst, dst_off, dst_cap, msg_res, res, max_message_size=0, src_len=None,
                         flags=0, stream=None):
    """websocketframeBatchInflateDevice (libwsframe_amd_deflate.so) on torch CUDA tensors: src (uint8,
    the compressed bodies), msg (uint8 >= 24*nseg*max_msgs: INFLATE_MSG_DTYPE records at s*max_msgs +
    i), nmsg (int32 nseg), dst (uint8: the rooms), dst_off / dst_cap (int64 nseg: connection s owns
    dst[dst_off[s]:dst_off[s] + dst_cap[s]]), msg_res (uint8 24*nseg*max_msgs: INFLATE_MSGRES_DTYPE),
    res (uint8 24*nseg: INFLATE_RES_DTYPE). src_len defaults to src.numel(); async on `stream`."""
    nseg = nmsg.numel()
    assert msg.numel() * msg.element_size() >= 24 * nseg * max_msgs
    assert msg_res.numel() * msg_res.element_size() >= 24 * nseg * max_msgs
    assert res.numel() * res.element_size() >= 24 * nseg
    assert dst_off.numel() * dst_off.element_size() >= 8 * nseg and dst_cap.numel() * dst_cap.element_size() >= 8 * nseg
    lib = _lib.load_deflate_lib()
    rc = lib.websocketframeBatchInflateDevice(_ptr(src), int(src.numel() if src_len is None else src_len), _ptr(msg), _ptr(nmsg),
                                              nseg, int(max_msgs), int(max_message_size), int(flags), _ptr(dst), _ptr(dst_off),
                                              _ptr(dst_cap), _ptr(msg_res), _ptr(res), _stream(stream))
    check(rc, "websocketframeBatchInflateDevice", lib)


def batch_inflate_list_from_messages_device(buf, desc, msg, nmsg, max_frames, inf_msg, stream=None):
    """websocketframeBatchInflateListFromMessagesDevice: the inflate list (uint8 >= 24*nseg*max_frames)
    from the wire buffer and what batch_reassemble_device left in desc, msg and nmsg; async on `stream`."""
    nseg = nmsg.numel()
    assert desc.numel() * desc.element_size() >= 32 * nseg * max_frames
    assert msg.numel() * msg.element_size() >= 32 * nseg * max_frames
    assert inf_msg.numel() * inf_msg.element_size() >= 24 * nseg * max_frames
    lib = _lib.load_deflate_lib()
    rc = lib.websocketframeBatchInflateListFromMessagesDevice(_ptr(buf), _ptr(desc), _ptr(msg), _ptr(nmsg), nseg,
                                                              int(max_frames), _ptr(inf_msg), _stream(stream))
    check(rc, "websocketframeBatchInflateListFromMessagesDevice", lib)


def inflate_host(src, msg, dst_cap, max_message_size=0, flags=0):
    """websocketframeInflateHost on one connection: src (numpy uint8), msg (INFLATE_MSG_DTYPE array).
    Returns (the connection's output bytes, INFLATE_MSGRES_DTYPE records, INFLATE_RES_DTYPE record)."""
    lib = _lib.load_deflate_lib()
    src = np.ascontiguousarray(src, dtype=np.uint8)
    msg = np.ascontiguousarray(msg, dtype=INFLATE_MSG_DTYPE)
    dst = np.zeros(max(1, dst_cap), np.uint8)
    mr = np.zeros(max(1, len(msg)), INFLATE_MSGRES_DTYPE)
    out = np.zeros(1, INFLATE_RES_DTYPE)
    n = lib.websocketframeInflateHost(src.ctypes.data if len(src) else None, len(src), msg.ctypes.data if len(msg) else None,
                                      len(msg), int(max_message_size), int(flags), dst.ctypes.data, int(dst_cap),
                                      mr.ctypes.data, out.ctypes.data)
    if n < 0:
        check(-1, "websocketframeInflateHost", lib)
    return bytes(dst[:n]), mr[:len(msg)], out[0]


def batch_deflate_device(src, msg, nmsg, max_msgs, dst, dst_off, dst_cap, msg_res, min_len=0, src_len=None, flags=0, stream=None):
    """websocketframeBatchDeflateDevice (libwsframe_amd_pmd.so) on torch CUDA tensors: src (uint8, the
    bodies), msg (uint8 >= 24*nseg*max_msgs: a send list, DEFLATE_MSG_DTYPE records at s*max_msgs +
    i), nmsg (int32 nseg), dst (uint8: the rooms), dst_off / dst_cap (int64 nseg*max_msgs: slot q owns
    dst[dst_off[q]:dst_off[q] + dst_cap[q]]), msg_res (uint8 24*nseg*max_msgs: DEFLATE_MSGRES_DTYPE).
    src_len defaults to src.numel(); async on `stream`."""
    nseg = nmsg.numel()
    assert msg.numel() * msg.element_size() >= 24 * nseg * max_msgs
    assert msg_res.numel() * msg_res.element_size() >= 24 * nseg * max_msgs
    assert dst_off.numel() * dst_off.element_size() >= 8 * nseg * max_msgs
    assert dst_cap.numel() * dst_cap.element_size() >= 8 * nseg * max_msgs
    lib = _lib.load_pmd_lib()
    rc = lib.websocketframeBatchDeflateDevice(_ptr(src), int(src.numel() if src_len is None else src_len), _ptr(msg), _ptr(nmsg),
                                              nseg, int(max_msgs), int(min_len), int(flags), _ptr(dst), _ptr(dst_off),
                                              _ptr(dst_cap), _ptr(msg_res), _stream(stream))
    check(rc, "websocketframeBatchDeflateDevice", lib)


def batch_send_list_from_deflated_device(msg, nmsg, max_msgs, msg_res, send_msg, stream=None):
    """websocketframeBatchSendListFromDeflatedDevice: the send list (uint8 >= 24*nseg*max_msgs) of what
    batch_deflate_device left in msg_res, DEFLATED entries marked SEND_TYPE_RSV1; async on `stream`."""
    nseg = nmsg.numel()
    assert msg.numel() * msg.element_size() >= 24 * nseg * max_msgs
    assert msg_res.numel() * msg_res.element_size() >= 24 * nseg * max_msgs
    assert send_msg.numel() * send_msg.element_size() >= 24 * nseg * max_msgs
    lib = _lib.load_pmd_lib()
    rc = lib.websocketframeBatchSendListFromDeflatedDevice(_ptr(msg), _ptr(nmsg), nseg, int(max_msgs), _ptr(msg_res),
                                                           _ptr(send_msg), _stream(stream))
    check(rc, "websocketframeBatchSendListFromDeflatedDevice", lib)


def batch_send_ext_device(src, msg, nmsg, max_msgs, tx, tx_off, send_res, frag_size=None, mask_key=None, msg_tx_off=None,
                          tx_capacity=None, src_len=None, flags=SEND_FLAG_RSV1, stream=None):
    """websocketframeBatchSendExtDevice (libwsframe_amd_pmd.so): batch_send_device's arguments; under
    flags = SEND_FLAG_RSV1 an entry whose type has SEND_TYPE_RSV1 carries RSV1 on its first frame."""
    nseg = nmsg.numel()
    assert msg.numel() * msg.element_size() >= 24 * nseg * max_msgs
    assert tx_off.numel() * tx_off.element_size() >= 8 * (nseg + 1)
    assert send_res.numel() * send_res.element_size() >= 32 * nseg
    assert frag_size is None or frag_size.numel() * frag_size.element_size() >= 4 * nseg
    assert mask_key is None or mask_key.numel() * mask_key.element_size() >= 4 * nseg * max_msgs
    assert msg_tx_off is None or msg_tx_off.numel() * msg_tx_off.element_size() >= 8 * nseg * max_msgs
    cap = (0 if tx is None else tx.numel()) if tx_capacity is None else tx_capacity
    lib = _lib.load_pmd_lib()
    rc = lib.websocketframeBatchSendExtDevice(_ptr(src), int(src.numel() if src_len is None else src_len), _ptr(msg), _ptr(nmsg),
                                              nseg, int(max_msgs), _ptr(frag_size), _ptr(mask_key), int(flags), _ptr(tx),
                                              int(cap), _ptr(tx_off), _ptr(msg_tx_off), _ptr(send_res), _stream(stream))
    check(rc, "websocketframeBatchSendExtDevice", lib)


def deflate_host(src, msg, dst_off, dst_cap, dst_len, min_len=0, flags=0, fill=0):
    """websocketframeDeflateHost on one list: src (numpy uint8), msg (DEFLATE_MSG_DTYPE array), dst_off /
    dst_cap (one room per entry, inside a destination of dst_len bytes preset to `fill`). Returns
    (the destination as a numpy array, DEFLATE_MSGRES_DTYPE records, the C return value)."""
    lib = _lib.load_pmd_lib()
    src = np.ascontiguousarray(src, dtype=np.uint8)
    msg = np.ascontiguousarray(msg, dtype=DEFLATE_MSG_DTYPE)
    off = np.ascontiguousarray(dst_off, dtype=np.uint64)
    cap = np.ascontiguousarray(dst_cap, dtype=np.uint64)
    assert len(off) == len(cap) == len(msg)
    dst = np.full(max(1, dst_len), fill, np.uint8)
    mr = np.zeros(max(1, len(msg)), DEFLATE_MSGRES_DTYPE)
    n = lib.websocketframeDeflateHost(src.ctypes.data if len(src) else None, len(src), msg.ctypes.data if len(msg) else None,
                                      len(msg), int(min_len), int(flags), dst.ctypes.data, off.ctypes.data if len(msg) else None,
                                      cap.ctypes.data if len(msg) else None, mr.ctypes.data if len(msg) else None)
    if n < 0:
        check(-1, "websocketframeDeflateHost", lib)
    return dst[:dst_len], mr[:len(msg)], n


def send_ext_host(src, msg, frag_size=SEND_FRAG_DEFAULT, mask_key=None, flags=SEND_FLAG_RSV1):
    """websocketframeSendExtHost on one connection (send_host's arguments, sized by a first call).
    Returns (the wire bytes, every message's offset, SEND_RES_DTYPE record)."""
    lib = _lib.load_pmd_lib()
    src = np.ascontiguousarray(src, dtype=np.uint8)
    msg = np.ascontiguousarray(msg, dtype=SEND_MSG_DTYPE)
    keys = None if mask_key is None else np.ascontiguousarray(mask_key, dtype=np.uint32)
    kp = None if keys is None else keys.ctypes.data
    out = np.zeros(1, SEND_RES_DTYPE)
    moff = np.zeros(max(1, len(msg)), np.uint64)
    sp = (src if len(src) else np.zeros(1, np.uint8)).ctypes.data
    n = lib.websocketframeSendExtHost(sp, len(src), msg.ctypes.data, len(msg), int(frag_size), kp, int(flags), None, 0, None,
                                      out.ctypes.data)
    if n < 0:
        check(-1, "websocketframeSendExtHost", lib)
    tx = np.zeros(max(1, n), np.uint8)
    n = lib.websocketframeSendExtHost(sp, len(src), msg.ctypes.data, len(msg), int(frag_size), kp, int(flags), tx.ctypes.data, n,
                                      moff.ctypes.data, out.ctypes.data)
    return bytes(tx[:n]), moff[:len(msg)], out[0]


def batch_handshake_device(buf, seg_off, seg_len, hs, flags=0, accept=None, resp=None, resp_off=None, resp_cap=0,
                           stream=None, buflen=None):
    """websocketframeBatchHandshakeDevice (libwsframe_amd_hs.so) on torch CUDA tensors: buf (uint8, only
    read; the last BATCH_PAD bytes are slack), seg_off/seg_len (int64 nseg), hs (uint8 32*nseg:
    HS_DTYPE records), accept (uint8 32*nseg, optional), resp (uint8, optional) with slots at
    resp_off (int64 nseg) or s*resp_cap. flags: 0 or HS_ECHO_PROTOCOL; async on `stream`. buflen
    defaults to buf.numel() - BATCH_PAD."""
    nseg = seg_off.numel()
    assert seg_len.numel() == nseg and hs.numel() * hs.element_size() >= 32 * nseg
    assert accept is None or accept.numel() * accept.element_size() >= 32 * nseg
    assert resp is None or resp_off is not None or resp.numel() >= nseg * resp_cap
    assert resp_off is None or resp_off.numel() >= nseg
    if buflen is None:
        assert buf.numel() >= BATCH_PAD, "device batch needs WEBSOCKET_BATCH_PAD bytes of slack"
        buflen = buf.numel() - BATCH_PAD
    lib = _lib.load_hs_lib()
    rc = lib.websocketframeBatchHandshakeDevice(_ptr(buf), int(buflen), _ptr(seg_off), _ptr(seg_len), nseg, int(flags),
                                                _ptr(hs), _ptr(accept), _ptr(resp), _ptr(resp_off), int(resp_cap),
                                                _stream(stream))
    check(rc, "websocketframeBatchHandshakeDevice", lib)


def handshake_host(data, flags=0, resp_cap=512, want_accept=True, want_resp=True):
    """websocketframeHandshakeHost on one request (bytes): returns (HS_DTYPE record, accept bytes
    (28) or None, response bytes or None). The request is copied into a buffer with BATCH_PAD
    bytes after it."""
    lib = _lib.load_hs_lib()
    buf = np.zeros(len(data) + BATCH_PAD, np.uint8)
    buf[:len(data)] = np.frombuffer(bytes(data), np.uint8)
    hs = np.zeros(1, HS_DTYPE)
    acc = np.zeros(32, np.uint8)
    resp = np.zeros(max(1, resp_cap), np.uint8)
    rc = lib.websocketframeHandshakeHost(buf.ctypes.data, len(data), int(flags), hs.ctypes.data,
                                         acc.ctypes.data if want_accept else None,
                                         resp.ctypes.data if want_resp else None, int(resp_cap))
    check(rc, "websocketframeHandshakeHost", lib)
    d = hs[0]
    ok = int(d["ret"]) > 0
    return (d, bytes(acc[:28]) if ok and want_accept else None,
            bytes(resp[:int(d["resp_len"])]) if int(d["flags"]) & HS_RESP_WRITTEN else None)


def batch_client_request_device(strs, entry, nonce, req, expect, rd, req_off=None, req_cap=0, flags=0, stream=None):
    """websocketframeBatchClientRequestDevice (libwsframe_amd_cli.so) on torch CUDA tensors: strs (uint8
    string pool), entry (uint8 48*nseg: CLI_ENTRY_DTYPE records), nonce (uint8 16*nseg), req (uint8)
    with slots at req_off (int64 nseg) or s*req_cap, expect (uint8 32*nseg), rd (uint8 16*nseg:
    CLI_REQ_DTYPE records); async on `stream`."""
    nseg = entry.numel() * entry.element_size() // CLI_ENTRY_DTYPE.itemsize
    assert nonce.numel() >= 16 * nseg and expect.numel() >= 32 * nseg and rd.numel() * rd.element_size() >= 16 * nseg
    assert req is None or req_off is not None or req.numel() >= nseg * req_cap
    assert req_off is None or req_off.numel() >= nseg
    lib = _lib.load_cli_lib()
    rc = lib.websocketframeBatchClientRequestDevice(_ptr(strs), strs.numel(), _ptr(entry), _ptr(nonce), nseg, int(flags),
                                                    _ptr(req), _ptr(req_off), int(req_cap), _ptr(expect), _ptr(rd),
                                                    _stream(stream))
    check(rc, "websocketframeBatchClientRequestDevice", lib)


def batch_client_verify_device(buf, seg_off, seg_len, expect, cv, strs=None, entry=None, max_head=0, flags=0, stream=None,
                               buflen=None):
    """websocketframeBatchClientVerifyDevice (libwsframe_amd_cli.so) on torch CUDA tensors: buf (uint8,
    only read; the last BATCH_PAD bytes are slack), seg_off/seg_len (int64 nseg), expect (uint8
    32*nseg, as the request call wrote it), cv (uint8 32*nseg: CLI_VERIFY_DTYPE records), strs and
    entry (optional: the offered subprotocols); async on `stream`. buflen defaults to
    buf.numel() - BATCH_PAD."""
    nseg = seg_off.numel()
    assert seg_len.numel() == nseg and cv.numel() * cv.element_size() >= 32 * nseg and expect.numel() >= 32 * nseg
    assert entry is None or (strs is not None and entry.numel() * entry.element_size() >= 48 * nseg)
    if buflen is None:
        assert buf.numel() >= BATCH_PAD, "device batch needs WEBSOCKET_BATCH_PAD bytes of slack"
        buflen = buf.numel() - BATCH_PAD
    lib = _lib.load_cli_lib()
    rc = lib.websocketframeBatchClientVerifyDevice(_ptr(buf), int(buflen), _ptr(seg_off), _ptr(seg_len), nseg, int(flags),
                                                   _ptr(expect), _ptr(strs), 0 if strs is None else strs.numel(),
                                                   _ptr(entry), int(max_head), _ptr(cv), _stream(stream))
    check(rc, "websocketframeBatchClientVerifyDevice", lib)


def client_request_host(path, nonce, proto=b"", host=b"", req_cap=4096, want_req=True, flags=0):
    """websocketframeClientRequestHost for one connection (bytes): returns (CLI_REQ_DTYPE record,
    request bytes or None, expect bytes (32) or None)."""
    lib = _lib.load_cli_lib()
    assert len(nonce) == 16
    arr = [np.frombuffer(bytes(b) + b"\0", np.uint8).copy() for b in (path, proto, host, nonce)]
    rd = np.zeros(1, CLI_REQ_DTYPE)
    req = np.zeros(max(1, req_cap), np.uint8)
    expect = np.zeros(32, np.uint8)
    rc = lib.websocketframeClientRequestHost(arr[0].ctypes.data, len(path), arr[1].ctypes.data, len(proto),
                                             arr[2].ctypes.data, len(host), arr[3].ctypes.data, int(flags),
                                             req.ctypes.data if want_req else None, int(req_cap), expect.ctypes.data,
                                             rd.ctypes.data)
    check(rc, "websocketframeClientRequestHost", lib)
    d = rd[0]
    err = int(d["flags"]) & (CLI_ERR_RANGE | CLI_ERR_BYTES)
    return (d, bytes(req[:int(d["req_len"])]) if int(d["flags"]) & CLI_REQ_WRITTEN else None,
            None if err else bytes(expect))


def client_verify_host(data, expect, offered=b"", max_head=0, flags=0):
    """websocketframeClientVerifyHost on one response (bytes): returns the CLI_VERIFY_DTYPE record. The
    response is copied into a buffer with BATCH_PAD bytes after it."""
    lib = _lib.load_cli_lib()
    buf = np.zeros(len(data) + BATCH_PAD, np.uint8)
    buf[:len(data)] = np.frombuffer(bytes(data), np.uint8)
    ex = np.frombuffer(bytes(expect).ljust(32, b"\0"), np.uint8).copy()
    of = np.frombuffer(bytes(offered) + b"\0", np.uint8).copy()
    cv = np.zeros(1, CLI_VERIFY_DTYPE)
    rc = lib.websocketframeClientVerifyHost(buf.ctypes.data, len(data), int(flags), ex.ctypes.data,
                                            of.ctypes.data if offered else None, len(offered), int(max_head),
                                            cv.ctypes.data)
    check(rc, "websocketframeClientVerifyHost", lib)
    return cv[0]


def batch_encode_device(src, frames, dst, wire_off, capacity=None, stream=None):
    """websocketframeBatchEncodeDevice on torch CUDA tensors: src (uint8 payload bytes),
    frames (uint8 tensor holding ENC_DTYPE records), dst (uint8), wire_off (int64,
    nframes + 1); async on `stream`. capacity defaults to dst.numel()."""
    n = frames.numel() // ENC_DTYPE.itemsize
    assert wire_off.numel() >= n + 1
    cap = dst.numel() if capacity is None else capacity
    rc = load_lib().websocketframeBatchEncodeDevice(_ptr(src), _ptr(frames), n, _ptr(dst), cap, _ptr(wire_off),
                                                    _stream(stream))
    check(rc, "websocketframeBatchEncodeDevice")


def batch_decode_host(buf, seg_off, seg_len, max_frames, device=0):
    """websocketframeBatchDecodeHost: buf (numpy uint8, modified in place), seg_off/seg_len
    (numpy uint64). Returns (desc structured array [nseg*max_frames], res [nseg])."""
    nseg = len(seg_off)
    seg_off = np.ascontiguousarray(seg_off, dtype=np.uint64)
    seg_len = np.ascontiguousarray(seg_len, dtype=np.uint64)
    desc = np.zeros(max(1, nseg * max_frames), dtype=DESC_DTYPE)
    res = np.zeros(max(1, nseg), dtype=SEGRES_DTYPE)
    rc = load_lib().websocketframeBatchDecodeHost(buf.ctypes.data, buf.nbytes, seg_off.ctypes.data,
                                                  seg_len.ctypes.data, nseg, max_frames, desc.ctypes.data,
                                                  res.ctypes.data, device)
    check(rc, "websocketframeBatchDecodeHost")
    return desc, res[:nseg]


def batch_decode_host_multi(buf, seg_off, seg_len, max_frames, devices):
    """websocketframeBatchDecodeHostMulti: buf (numpy uint8, modified in place) decoded on several
    devices (a byte-balanced range each; a device may repeat). Returns (desc, res) as
    batch_decode_host does."""
    nseg = len(seg_off)
    seg_off = np.ascontiguousarray(seg_off, dtype=np.uint64)
    seg_len = np.ascontiguousarray(seg_len, dtype=np.uint64)
    desc = np.zeros(max(1, nseg * max_frames), dtype=DESC_DTYPE)
    res = np.zeros(max(1, nseg), dtype=SEGRES_DTYPE)
    devs = np.ascontiguousarray(devices, dtype=np.int32)
    rc = load_lib().websocketframeBatchDecodeHostMulti(buf.ctypes.data, buf.nbytes, seg_off.ctypes.data,
                                                       seg_len.ctypes.data, nseg, max_frames, desc.ctypes.data,
                                                       res.ctypes.data, devs.ctypes.data, len(devs))
    check(rc, "websocketframeBatchDecodeHostMulti")
    return desc, res[:nseg]


def synth_device(buf, frame_off, nframes, plen_kind, fixed_len, b0_kind, seed, stream=None, first_frame=0):
    """websocketframeSynthDeviceRange (libwsframe_amd_bench.so): bench/test input generated in
    HBM — generator frames first_frame .. first_frame + nframes - 1 at buf + frame_off[i]"""
    rc = load_bench_lib().websocketframeSynthDeviceRange(_ptr(buf), _ptr(frame_off), first_frame, nframes, plen_kind,
                                                         fixed_len, b0_kind, seed, _stream(stream))
    check_bench(rc, "websocketframeSynthDeviceRange")


def synth_verify_device(buf, frame_off, nframes, plen_kind, fixed_len, seed, expect_plain, mismatch, stream=None,
                        first_frame=0):
    rc = load_bench_lib().websocketframeSynthVerifyDeviceRange(_ptr(buf), _ptr(frame_off), first_frame, nframes,
                                                               plen_kind, fixed_len, seed, 1 if expect_plain else 0,
                                                               _ptr(mismatch), _stream(stream))
    check_bench(rc, "websocketframeSynthVerifyDeviceRange")


def frame_hash_device(buf, desc, res, nseg, max_frames, out, stream=None):
    """websocketframeFrameHashDevice: adds the decoded batch's output hash into out (int64 CUDA
    tensor, one element, u64 wrap-around)"""
    rc = load_bench_lib().websocketframeFrameHashDevice(_ptr(buf), _ptr(desc), _ptr(res), nseg, max_frames, _ptr(out),
                                                        _stream(stream))
    check_bench(rc, "websocketframeFrameHashDevice")


def set_option(name, value):
    """websocketframeGpuSetOption (launch tuning knobs, for A/B measurement)"""
    rc = _lib.set_option(name, value)          # both libraries
    if rc != 0:
        raise ValueError("unknown option %r" % name)


def get_stat(name):
    """websocketframeGpuGetStat (diagnostic counters of the most recent call)"""
    v = C.c_ulonglong(0)
    if load_lib().websocketframeGpuGetStat(name.encode(), C.byref(v)) != 0:
        raise ValueError("unknown stat %r" % name)
    return int(v.value)
