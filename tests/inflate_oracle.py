"""The sequential model of websocketframeBatchInflateDevice / websocketframeInflateHost
(include/wsframe_amd_deflate.h). The inflater is CPython's zlib: a message's input is its body plus
00 00 FF FF, its output what zlib.decompressobj(-15).decompress() returns, its verdict whether that
raises. The model packs the outputs per connection and applies first failure and NOT_RUN."""
import functools
import zlib

import numpy as np

MSG_DTYPE = np.dtype([("src_off", "<u8"), ("len", "<u8"), ("kind", "<u4"), ("reserved", "<u4")])
MSGRES_DTYPE = np.dtype([("out_off", "<u8"), ("out_len", "<u8"), ("status", "<u4"), ("reserved", "<u4")])
RES_DTYPE = np.dtype([("out_len", "<u8"), ("n_msgs", "<u4"), ("status", "<u4"), ("first_bad", "<u4"),
                      ("close_status", "<u4")])
assert MSG_DTYPE.itemsize == MSGRES_DTYPE.itemsize == RES_DTYPE.itemsize == 24
SKIP = NONE = 0xFFFFFFFF
RAW = 1
OK, ERR_DATA, ERR_TOO_BIG, ERR_OUT_SPACE, ERR_RANGE, NOT_RUN = range(6)
CLOSE = {ERR_DATA: 1007, ERR_TOO_BIG: 1009}
TAIL = b"\x00\x00\xff\xff"
FILL = 0xA5


@functools.lru_cache(maxsize=None)
def inflate_one(body, limit=0):
    """(status before the room is looked at, output): ERR_DATA where zlib raises within limit + 1
    output bytes, else ERR_TOO_BIG where it returns more than limit"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(body + TAIL, limit + 1) if limit else d.decompress(body + TAIL)
    except zlib.error:
        return ERR_DATA, b""
    if limit and len(out) > limit:
        return ERR_TOO_BIG, b""
    return OK, out


def connection(src, msgs, limit, base, cap):
    """one connection's list [(src_off, len, kind)] -> (MSGRES records, RES record, its output bytes)"""
    src = bytes(src)
    mr = np.zeros(len(msgs), MSGRES_DTYPE)
    res = np.zeros(1, RES_DTYPE)[0]
    res["first_bad"] = NONE
    out = b""
    for i, (off, ln, kind) in enumerate(msgs):
        mr[i]["out_off"] = base + len(out)
        if res["status"] != OK:
            mr[i]["status"] = NOT_RUN
            continue
        if kind == SKIP:
            continue
        if kind != RAW or off + ln > len(src):
            st, body = ERR_RANGE, b""
        else:
            st, body = inflate_one(src[off:off + ln], limit)
            if st == OK and len(body) > cap - len(out):
                st, body = ERR_OUT_SPACE, b""
        mr[i]["status"] = st
        if st == OK:
            mr[i]["out_len"] = len(body)
            out += body
            res["n_msgs"] += 1
        else:
            res["status"], res["first_bad"], res["close_status"] = st, i, CLOSE.get(st, 0)
    res["out_len"] = len(out)
    return mr, res, out


def batch(src, msg, nmsg, max_msgs, limit, dst_off, dst_cap, fill=0xEE):
    """the whole call: (MSGRES [nseg*max_msgs] with unwritten slots left at `fill` bytes, RES [nseg],
    [every connection's output bytes])"""
    nseg = len(nmsg)
    src = bytes(src)                                          # once: connection() takes bytes as they are
    mr = np.frombuffer(bytes([fill]) * (24 * nseg * max_msgs), MSGRES_DTYPE).copy()
    res = np.zeros(nseg, RES_DTYPE)
    outs = []
    for s in range(nseg):
        n = min(int(nmsg[s]), max_msgs)
        lst = [(int(m["src_off"]), int(m["len"]), int(m["kind"])) for m in msg[s * max_msgs:s * max_msgs + n]]
        r, res[s], out = connection(src, lst, limit, int(dst_off[s]), int(dst_cap[s]))
        mr[s * max_msgs:s * max_msgs + n] = r
        outs.append(out)
    return mr, res, outs
