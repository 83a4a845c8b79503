"""Sequential oracle of the protocol check (include/wsframe_amd_proto.h), written from the rule
frame by frame with running variables: no scan, no summary, no project library. It takes the
descriptors, the segment results and the wire of one batch and returns every frame's code, the
per-segment result records and the state words."""
import numpy as np

OK, ERR_RSV, ERR_OPCODE, ERR_MASK, ERR_CTL_FRAGMENTED, ERR_CTL_LENGTH, ERR_CLOSE_LENGTH, ERR_CLOSE_CODE, \
    ERR_CONT_UNEXPECTED, ERR_DATA_INTERLEAVED, ERR_TOO_BIG = range(11)
AFTER_CLOSE, NOT_CONSUMED = 0x80, 0x81
EXPECT_MASKED, EXPECT_UNMASKED, WIRE_MASKED = 1, 2, 4
NONE = 0xFFFFFFFF
ST_OPEN, ST_CLOSED, BYTES_MAX = 1 << 63, 1 << 62, (1 << 56) - 1
FILL = 0xEE

RES_DTYPE = np.dtype([("first_bad", "<u4"), ("code", "<u4"), ("close_status", "<u4"), ("close_frame", "<u4")])


def close_code_ok(c):
    return 1000 <= c <= 1003 or 1007 <= c <= 1014 or 3000 <= c <= 4999


class Conn:
    """one connection: the running variables of the rule"""

    def __init__(self, state=0):
        self.open = bool(state & ST_OPEN)
        self.closed = bool(state & ST_CLOSED)
        self.bytes = state & BYTES_MAX

    def word(self):
        return (ST_OPEN if self.open else 0) | (ST_CLOSED if self.closed else 0) | (self.bytes if self.open else 0)

    def frame(self, b0, typ, fin, masked, datalen, body2, flags, rsv_allowed, limit):
        """code of one consumed frame (typ, fin: the descriptor's fields; body2: the two unmasked
        status bytes of a CLOSE, or None); moves the connection past it"""
        if self.closed:
            return AFTER_CLOSE
        code = self.judge(b0, typ, fin, masked, datalen, body2, flags, rsv_allowed, limit)
        if typ == 8:
            self.closed = True
        if not typ & 8:                                   # a data frame, in error or not
            if fin:
                self.open, self.bytes = False, 0
            else:
                self.open, self.bytes = True, min(self.bytes + min(datalen, BYTES_MAX), BYTES_MAX)
        return code

    def judge(self, b0, typ, fin, masked, datalen, body2, flags, rsv_allowed, limit):
        if b0 & 0x70 & ~rsv_allowed:
            return ERR_RSV
        if 3 <= typ <= 7 or 11 <= typ <= 15:
            return ERR_OPCODE
        if (flags & EXPECT_MASKED and not masked) or (flags & EXPECT_UNMASKED and masked):
            return ERR_MASK
        if typ & 8:
            if not fin:
                return ERR_CTL_FRAGMENTED
            if datalen > 125:
                return ERR_CTL_LENGTH
            if typ == 8 and datalen == 1:
                return ERR_CLOSE_LENGTH
            if typ == 8 and datalen >= 2 and not close_code_ok(body2[0] << 8 | body2[1]):
                return ERR_CLOSE_CODE
            return OK
        if typ == 0 and not self.open:
            return ERR_CONT_UNEXPECTED
        if typ != 0 and self.open:
            return ERR_DATA_INTERLEAVED
        if limit and min(self.bytes + min(datalen, BYTES_MAX), BYTES_MAX) > limit:
            return ERR_TOO_BIG
        return OK


def check(wire, seg_off, desc, res, max_frames, flags=0, rsv_allowed=0, limit=0, state=None):
    """The whole batch. wire: uint8 array; desc: DESC_DTYPE records at s*max_frames + k; res:
    SEGRES_DTYPE records; state: the incoming words (None: every batch stands alone). Returns
    (codes uint8 [nseg*max_frames], FILL where nothing is written; result records; state words
    out, the incoming ones when state is None ... never stored then: None)."""
    nseg = len(seg_off)
    codes = np.full(nseg * max_frames, FILL, np.uint8)
    out = np.zeros(nseg, RES_DTYPE)
    words = None if state is None else np.zeros(nseg, np.uint64)
    for s in range(nseg):
        conn = Conn(0 if state is None else int(state[s]))
        was_closed = conn.closed
        end = int(seg_off[s]) + int(res[s]["consumed"])
        first_bad, bad_code, close_frame = NONE, 0, NONE
        for k in range(min(int(res[s]["n_frames"]), max_frames)):
            d = desc[s * max_frames + k]
            ret, fo = int(d["ret"]), int(d["frame_off"])
            if not (ret > 0 and fo + ret <= end):
                codes[s * max_frames + k] = NOT_CONSUMED
                continue
            typ, datalen, masked = int(d["type"]), int(d["datalen"]), int(d["masked"])
            body2 = None
            if typ == 8 and datalen >= 2 and not conn.closed:
                do = int(d["data_off"])
                body2 = [int(wire[do]), int(wire[do + 1])]
                if flags & WIRE_MASKED and masked:
                    body2 = [body2[0] ^ int(wire[do - 4]), body2[1] ^ int(wire[do - 3])]
            if typ == 8 and not conn.closed:
                close_frame = k
            code = conn.frame(int(wire[fo]), typ, int(d["is_fin"]), masked, datalen, body2, flags, rsv_allowed, limit)
            codes[s * max_frames + k] = code
            if 1 <= code <= 10 and first_bad == NONE:
                first_bad, bad_code = k, code
        status = 0 if first_bad == NONE else (1009 if bad_code == ERR_TOO_BIG else 1002)
        out[s] = (first_bad, bad_code, status, NONE if was_closed else close_frame)
        if words is not None:
            words[s] = conn.word()
    return codes, out, words
