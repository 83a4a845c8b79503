"""The model the deflate tests hold the library against (test_deflate_host.py, test_gpu_deflate.py).

The compressor is free in what it finds, so the oracle does not predict bytes: it judges them. A
DEFLATED body must inflate, through CPython's zlib, to the original; a PLAIN room must hold the
original; and the verdict must follow include/wsframe_amd_compress.h's rule from the encoded length
the rule reported. tokens() is a small fixed-Huffman reader of its own, for what zlib does not tell:
the block's shape, every match's length and distance. send_ext() is the host model of the ext send:
send_oracle's wire bytes with 0x40 set on the first frame of every entry marked RSV1."""
import zlib

import numpy as np

import send_oracle as S

DEFLATED, PLAIN, SKIPPED, ERR_OUT_SPACE, ERR_RANGE = range(5)
SKIP = 0xFFFFFFFF
FILL = 0xA7
TAIL = b"\x00\x00\xff\xff"
RSV1_TYPE, RSV1_FLAG = 0x40, 1
MSG_DTYPE = S.MSG_DTYPE
MSGRES_DTYPE = np.dtype([("out_off", "<u8"), ("out_len", "<u8"), ("status", "<u4"), ("reserved", "<u4")])


def inflate(body):
    return zlib.decompressobj(-15).decompress(bytes(body) + TAIL)


def verdict(n, min_len, cap, enc_len):
    """(status, out_len) of a message of n bytes whose encoding, when it is encoded, has enc_len bytes"""
    if n == 0 or n < min_len:
        return (PLAIN, n) if n <= cap else (ERR_OUT_SPACE, 0)
    if enc_len < n and enc_len <= cap:
        return DEFLATED, enc_len
    return (PLAIN, n) if n <= cap else (ERR_OUT_SPACE, 0)


def judge(data, min_len, cap, status, out_len, room, enc_len=None, tag=""):
    """one entry that ran: `room` the cap bytes of its room after the call. enc_len: what the rule
    reported (the host build tells; without it the verdict is checked as far as the result shows)."""
    n = len(data)
    coded = n > 0 and n >= min_len
    if enc_len is not None:
        assert (status, out_len) == verdict(n, min_len, cap, enc_len), "%s: %s, enc_len %d" % (tag, (status, out_len), enc_len)
        assert coded or enc_len == 0, tag
    if status == DEFLATED:
        assert coded and out_len < n and out_len <= cap, tag
        assert inflate(room[:out_len]) == data, tag + ": the body does not inflate to the message"
    elif status == PLAIN:
        assert out_len == n <= cap and bytes(room[:n]) == data, tag
    else:
        assert status == ERR_OUT_SPACE and out_len == 0 and n > cap, tag


class _Bits:
    def __init__(self, body):
        self.v, self.n, self.at = int.from_bytes(body, "little"), 8 * len(body), 0

    def take(self, k):
        assert self.at + k <= self.n, "the stream ends inside a symbol"
        r = (self.v >> self.at) & ((1 << k) - 1)
        self.at += k
        return r

    def code(self, k):                                     # k bits, most significant first
        r = 0
        for _ in range(k):
            r = r << 1 | self.take(1)
        return r


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def tokens(body):
    """the tokens of a body the rule wrote: ints (literals) and (length, distance) pairs. Asserts the
    shape: one fixed block with BFINAL 0, the end-of-block code, 000, zero padding to the byte."""
    b = _Bits(bytes(body))
    assert b.take(1) == 0 and b.take(2) == 1, "not one fixed-Huffman block with BFINAL 0"
    out = []
    while True:
        c = b.code(7)
        if c <= 0x17:
            sym = 256 + c
        else:
            c = c << 1 | b.take(1)
            if 0x30 <= c <= 0xBF:
                sym = c - 0x30
            elif 0xC0 <= c <= 0xC7:
                sym = 280 + c - 0xC0
            else:
                c = c << 1 | b.take(1)
                assert 0x190 <= c <= 0x1FF
                sym = 144 + c - 0x190
        if sym < 256:
            out.append(sym)
            continue
        if sym == 256:
            break
        assert sym <= 285
        length = LEN_BASE[sym - 257] + b.take(LEN_EXTRA[sym - 257])
        d = b.code(5)
        assert d < 30
        out.append((length, DIST_BASE[d] + b.take(DIST_EXTRA[d])))
    assert b.take(3) == 0, "no empty stored block's header behind the end-of-block code"
    assert b.n - b.at < 8 and b.take(b.n - b.at) == 0, "more than zero padding to the byte"
    return out


def replay(toks):
    """the message the tokens stand for; every match inside the rule's limits"""
    out = bytearray()
    for t in toks:
        if isinstance(t, tuple):
            length, dist = t
            assert 4 <= length <= 258 and 1 <= dist <= 32768 and dist <= len(out), t
            for _ in range(length):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out)


def send_entry(typ, status, out_off, out_len):
    """websocketframeBatchSendListFromDeflatedDevice's map of one slot"""
    if typ == SKIP or status not in (DEFLATED, PLAIN):
        return (0, 0, SKIP)
    return (out_off, out_len, typ | RSV1_TYPE if status == DEFLATED else typ)


def send_ext(src, conns, frags=None, keys=None, max_msgs=None, flags=RSV1_FLAG):
    """S.batch's results for the ext send: under the flag, 0x40 on the first wire byte of every
    sent entry whose type has it — the first frame's, and no other frame's"""
    etx, eoff, emoff, eres = S.batch(src, conns, frags, keys, max_msgs)
    etx = np.array(etx, np.uint8)
    mm = max_msgs or max([1] + [len(c) for c in conns])
    if flags & RSV1_FLAG:
        for s, c in enumerate(conns):
            if int(eres[s]["status"]) != S.OK:
                continue
            for i, (_o, _n, t) in enumerate(c[:mm]):
                if t != SKIP and t & RSV1_TYPE:
                    etx[int(emoff[s * mm + i])] |= 0x40
    return etx, eoff, emoff, eres
