"""Sequential model of the batch message send (include/wsframe_amd_send.h) — TEST INFRASTRUCTURE ONLY.

One connection at a time, one message at a time: the reference's sharding loop
(channelbaseShardDatas, net_reactor.c:886-923, as a stream channel runs it after
NetChannelEx_init: write_fragment_with_hdr = 1, on_hdrsize = the frame header length) written out
line by line, and per packet the header the websocket on_pre_send glue writes: the oracle's
restatement of websocketframeEncode(hdr, fragment_eof, the previous packet's fragment_eof, type,
bodylen). The client role (MASK bit, key bytes, XORed body, one derived key per fragment) is this
project's addition and is modelled here as include/wsframe_amd_send.h words it."""
import ctypes as C

import numpy as np

from oracle_lib import load_oracle

SKIP = NONE = FRAG_DEFAULT = 0xFFFFFFFF
OK, ERR_FRAGMENT_SIZE, ERR_RANGE = 0, 1, 2
FILL = 0xEE
MSG_DTYPE = np.dtype([("src_off", "<u8"), ("len", "<u8"), ("type", "<u4"), ("reserved", "<u4")])
RES_DTYPE = np.dtype([("tx_len", "<u8"), ("n_frames", "<u8"), ("n_msgs", "<u4"), ("status", "<u4"),
                      ("first_bad", "<u4"), ("reserved", "<u4")])


def hdrsize(n, role):
    """on_hdrsize: websocketframeEncodeHeadLength, plus the key bytes in the client role"""
    return load_oracle().ws_oracle_encode_headlen(n) + (4 if role else 0)


def frag_key(key, j):
    """ws_send_frag_key: the key of fragment j of a message"""
    return (key ^ (j * 0x9E3779B9)) & 0xFFFFFFFF


def shard_packets(nbytes, F, role):
    """net_reactor.c:883-940: the (hdrsz, bodylen, fragment_eof) of every packet of one send of
    nbytes body bytes on a channel with write_fragment_size F; None where the reference returns NULL"""
    pk = []
    if nbytes:
        off = 0
        write_fragment_size = F
        shardsz = write_fragment_size
        hdrsz = hdrsize(shardsz, role)
        if shardsz <= hdrsz:
            return None
        shardsz -= hdrsz
        while off < nbytes:
            sz = nbytes - off
            if sz > shardsz:
                sz = shardsz
            hdrsz = hdrsize(sz, role)
            pk.append([hdrsz, sz, 0])
            off += sz
            # write_fragment_with_hdr: continue
        pk[-1][2] = 1
    else:
        pk.append([hdrsize(0, role), 0, 1])
    return pk


def shard_of(F, role):
    h = hdrsize(F, role)
    return 0 if F <= h else F - h


def message_wire(body, typ, F, key=None):
    """the wire bytes of one message (body: numpy uint8) and its frame count; None: NULL"""
    lib = load_oracle()
    role = key is not None
    pk = shard_packets(len(body), F, role)
    if pk is None:
        return None
    out, off, prev = [], 0, 1
    for j, (hdrsz, sz, eof) in enumerate(pk):
        h = (C.c_ubyte * 10)()
        lib.ws_oracle_encode(h, eof, prev, typ & 0x0F, sz)
        hb = bytearray(bytes(h)[:hdrsz - (4 if role else 0)])
        part = body[off:off + sz]
        if role:
            kb = frag_key(key, j).to_bytes(4, "little")
            hb[1] |= 0x80
            hb += kb
            part = part ^ np.resize(np.frombuffer(kb, np.uint8), sz)
        out.append(np.frombuffer(bytes(hb), np.uint8))
        out.append(part)
        off += sz
        prev = eof
    return np.concatenate(out), len(pk)


def connection(src, msgs, F=FRAG_DEFAULT, keys=None):
    """one connection's list: msgs = [(src_off, len, type)], keys = one u32 per message or None.
    Returns (wire bytes, every message's offset in them, (tx_len, n_frames, n_msgs, status, first_bad))."""
    role = keys is not None
    parts, offs, frames, nm, pos = [], [], 0, 0, 0
    for i, (so, ln, typ) in enumerate(msgs):
        offs.append(pos)
        if typ == SKIP:
            continue
        if so + ln > len(src):
            return np.zeros(0, np.uint8), [0] * len(msgs), (0, 0, 0, ERR_RANGE, i)
        got = message_wire(src[so:so + ln], typ, F, int(keys[i]) if role else None)
        if got is None:
            return np.zeros(0, np.uint8), [0] * len(msgs), (0, 0, 0, ERR_FRAGMENT_SIZE, i)
        parts.append(got[0])
        frames += got[1]
        nm += 1
        pos += len(got[0])
    tx = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return tx, offs, (len(tx), frames, nm, OK, NONE)


def batch(src, conns, frags=None, keys=None, max_msgs=None):
    """every connection of a batch: conns[s] = [(src_off, len, type)], frags[s] or None, keys as
    d_mask_key (numpy uint32 nseg*max_msgs) or None. Returns (tx bytes, tx_off u64 nseg + 1,
    msg_tx_off u64 nseg*max_msgs with NONE64 in the slots the call does not write, RES_DTYPE nseg)."""
    nseg = len(conns)
    max_msgs = max_msgs or max([1] + [len(c) for c in conns])
    tx_off = np.zeros(nseg + 1, np.uint64)
    moff = np.full(nseg * max_msgs, 0xEEEEEEEEEEEEEEEE, np.uint64)
    res = np.zeros(nseg, RES_DTYPE)
    parts, pos = [], 0
    for s, msgs in enumerate(conns):
        k = None if keys is None else keys[s * max_msgs:(s + 1) * max_msgs]
        tx, offs, r = connection(src, msgs, FRAG_DEFAULT if frags is None else int(frags[s]), k)
        tx_off[s] = pos
        for i, o in enumerate(offs):
            moff[s * max_msgs + i] = pos + o
        res[s] = r + (0,)
        parts.append(tx)
        pos += len(tx)
    tx_off[nseg] = pos
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), tx_off, moff, res


def pack(conns, max_msgs=None):
    """d_msg and d_nmsg of a batch: (SEND_MSG records nseg*max_msgs, filled with a poison entry
    past each count; u32 counts; max_msgs)"""
    nseg = len(conns)
    max_msgs = max_msgs or max([1] + [len(c) for c in conns])
    msg = np.zeros(nseg * max_msgs, MSG_DTYPE)
    msg["src_off"], msg["len"], msg["type"] = 1 << 60, 1 << 60, 2          # never read: past the count
    for s, c in enumerate(conns):
        for i, (so, ln, typ) in enumerate(c):
            msg[s * max_msgs + i] = (so, ln, typ, 0)
    return msg, np.array([len(c) for c in conns], np.uint32), max_msgs


def closed_form(L, F, role):
    """(frames, wire bytes) of a message, written out independently of the loop; None: NULL"""
    H = lambda n: (2 if n < 126 else 4 if n <= 0xFFFF else 10) + (4 if role else 0)
    if L == 0:
        return 1, H(0)
    if F <= H(F):
        return None
    shard = F - H(F)
    n = -(-L // shard)
    last = L - (n - 1) * shard
    return n, (n - 1) * (H(shard) + shard) + H(last) + last
