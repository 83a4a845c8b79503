"""Sequential model of the control replies (include/wsframe_amd_reply.h), written from the rule
segment by segment and frame by frame with running variables: no scan, no summary, no project
library. It takes the descriptors, the segment results and the wire of one batch and returns the
reply bytes, their offsets, the per-segment result records and the state words."""
import numpy as np

CLOSE_NONE, CLOSE_ECHO, CLOSE_PROTOCOL, CLOSE_CALLER = range(4)
WIRE_MASKED, LAST_PING_ONLY = 4, 8
ST_CLOSE_SENT = 1
NONE = 0xFFFFFFFF
FILL = 0xEE

RES_DTYPE = np.dtype([("n_pong", "<u4"), ("close_kind", "<u4"), ("close_status", "<u4"), ("tx_len", "<u4")])


def reply_frame(b0, body, key):
    """one reply frame: key None (server role) or the u32 whose byte i, low byte first, goes i-th on the wire"""
    if key is None:
        return bytes([b0, len(body)]) + bytes(body)
    kb = int(key).to_bytes(4, "little")
    return bytes([b0, 0x80 | len(body)]) + kb + bytes(b ^ kb[i & 3] for i, b in enumerate(body))


def body_bytes(wire, d, n, flags):
    """the first n unmasked body bytes of the frame with descriptor d"""
    do = int(d["data_off"])
    raw = [int(wire[do + i]) for i in range(n)]
    if flags & WIRE_MASKED and int(d["masked"]):
        raw = [b ^ int(wire[do - 4 + (i & 3)]) for i, b in enumerate(raw)]
    return bytes(raw)


def segment(wire, seg_off, desc, res, max_frames, flags, proto, fail, keys, state):
    """one segment: desc its max_frames slots, proto (first_bad, close_status) or None, keys its
    max_frames + 1 keys or None. Returns (reply bytes, result tuple, state out, the reply's frames
    as (opcode, fin, plain body))."""
    if state & ST_CLOSE_SENT:
        return b"", (0, 0, 0, 0), state, []
    b = NONE if proto is None else int(proto[0])
    end = int(seg_off) + int(res["consumed"])
    pings, c = [], NONE
    for k in range(min(int(res["n_frames"]), max_frames)):
        d = desc[k]
        ret = int(d["ret"])
        if not (ret > 0 and int(d["frame_off"]) + ret <= end):
            continue
        if int(d["type"]) == 8:
            c = k
            break
        if k < b and int(d["type"]) == 9 and int(d["is_fin"]) and int(d["datalen"]) <= 125:
            pings.append(k)
    if flags & LAST_PING_ONLY:
        pings = pings[-1:]
    tx, sent = b"", []
    for k in pings:
        sent.append((10, 1, body_bytes(wire, desc[k], int(desc[k]["datalen"]), flags)))
        tx += reply_frame(0x8A, sent[-1][2], None if keys is None else keys[k])
    kind, status, body = CLOSE_NONE, 0, None
    if b != NONE and b <= c:
        kind, status = CLOSE_PROTOCOL, int(proto[1]) & 0xFFFF
        body = status.to_bytes(2, "big")
    elif fail:
        kind, status = CLOSE_CALLER, int(fail) & 0xFFFF
        body = status.to_bytes(2, "big")
    elif c != NONE:
        kind = CLOSE_ECHO
        body = body_bytes(wire, desc[c], 2, flags) if int(desc[c]["datalen"]) >= 2 else b""
        status = int.from_bytes(body, "big") if body else 0
    if kind:
        sent.append((8, 1, body))
        tx += reply_frame(0x88, body, None if keys is None else keys[max_frames])
        state |= ST_CLOSE_SENT
    return tx, (len(pings), kind, status, len(tx)), state, sent


def replies(wire, seg_off, desc, res, max_frames, flags=0, proto_res=None, fail_status=None, keys=None, state=None):
    """The whole batch. proto_res: records with first_bad / close_status, or None; fail_status: u32
    per segment or None; keys: u32 [nseg * (max_frames + 1)] or None; state: the incoming words
    (None: every batch stands alone, nothing stored). Returns (all reply bytes, tx_off u64
    [nseg + 1], result records, state words out or None)."""
    nseg = len(seg_off)
    out = np.zeros(nseg, RES_DTYPE)
    off = np.zeros(nseg + 1, np.uint64)
    words = None if state is None else np.zeros(nseg, np.uint32)
    tx = b""
    for s in range(nseg):
        t, r, st, _ = segment(wire, seg_off[s], desc[s * max_frames:(s + 1) * max_frames], res[s], max_frames, flags,
                              None if proto_res is None else (proto_res[s]["first_bad"], proto_res[s]["close_status"]),
                              0 if fail_status is None else int(fail_status[s]),
                              None if keys is None else keys[s * (max_frames + 1):(s + 1) * (max_frames + 1)],
                              0 if state is None else int(state[s]))
        out[s] = r
        tx += t
        off[s + 1] = len(tx)
        if words is not None:
            words[s] = st
    return tx, off, out, words
