"""Checker for websocketframeBatchReassembleDeviceCtl with WEBSOCKET_REASM_CONTROL_DIRECT —
test infrastructure only.

The decode oracle (tests/oracle_lib.py, pinned to the reference's golden vectors) plus the
stream hook's delivery rule under a glue that leaves pktype = 0 for control frames
(net_channel_ex.c:125-126, 155), pinned to the reference's own reactor by
tests/golden/reassemble_ctl.json: a control frame (consumed, type & 8) is one message of its
own and touches neither the pending message nor the fragment cache; the other (data) frames
follow oracle_lib.oracle_reassemble's rule among themselves.
"""
import numpy as np

from oracle_lib import cache_overflow, oracle_segments


def oracle_reassemble_ctl(wire, seg_off, seg_len, max_frames, open_in=None, out_off=None, readcache_max=0,
                          cached_in=None):
    """Returns (desc, res, msgs[s] = [(out_off, len, first, n, complete, continued)] in delivery
    order, regions[s] = (out_off, data bodies upward from the region's start, control bodies as
    they lie at the region's end: the last one first), open_out, cached_out)."""
    buf = np.asarray(wire, dtype=np.uint8).copy()
    desc, res = oracle_segments(buf, seg_off, seg_len, max_frames)
    res = res.copy()
    msgs, regions, open_out, cached_out = [], [], [], []
    for s in range(len(seg_off)):
        ob = int(out_off[s]) if out_off is not None else int(seg_off[s])
        sl = int(seg_len[s])
        opened = int(open_in[s]) if open_in is not None else 0
        cached = int(cached_in[s]) & 0xFFFFFFFF if (cached_in is not None and opened) else 0
        cont, first, nmine, q, q0, qc = opened, 0, 0, 0, 0, 0
        data, ctl, ms = [], [], []
        for k in range(int(res[s]["n_frames"])):
            d = desc[s * max_frames + k]
            if int(d["ret"]) <= 0:
                break
            n = int(d["datalen"])
            if n > sl - (q + qc):                                      # all bodies before it
                res[s]["status"] = -3
                break
            a = int(d["data_off"])
            body = buf[a:a + n] if n else buf[:0]
            if int(d["type"]) & 8:                                     # control: straight to on_recv
                qc += n
                ctl.append(body)
                ms.append((ob + sl - qc, n, k, 1, 1, 0))
                continue
            fin = int(d["is_fin"])
            cache_it = bool(opened) or not fin                         # net_channel_ex.c:129
            if cache_it and cache_overflow(cached, n & 0xFFFFFFFF, readcache_max):
                res[s]["status"] = -4
                res[s]["consumed"] = int(d["frame_off"]) - int(seg_off[s])
                res[s]["n_frames"] = k + 1
                break
            if nmine == 0:
                first = k
            nmine += 1
            data.append(body)
            q += n
            if cache_it:
                cached = (cached + (n & 0xFFFFFFFF)) & 0xFFFFFFFF
            opened = 1
            if fin:
                ms.append((ob + q0, q - q0, first, nmine, 1, cont))
                nmine, q0, cont, opened, cached = 0, q, 0, 0, 0
        if opened and nmine:
            ms.append((ob + q0, q - q0, first, nmine, 0, cont))
        msgs.append(ms)
        empty = np.zeros(0, np.uint8)
        regions.append((ob, np.concatenate(data) if data else empty, np.concatenate(ctl[::-1]) if ctl else empty))
        open_out.append(opened)
        cached_out.append(cached if opened else 0)
    return desc, res, msgs, regions, np.array(open_out, dtype=np.uint8), np.array(cached_out, dtype=np.uint32)


def region_image(region, seg_len, fill=0xEE):
    """the seg_len bytes of a segment's output region: data bodies, untouched fill, control bodies"""
    _, data, ctl = region
    img = np.full(int(seg_len), fill, np.uint8)
    img[:len(data)] = data
    if len(ctl):
        img[len(img) - len(ctl):] = ctl
    return img


def reactor_view_ctl(msgs, regions, res, open_out, cached_out, seg_len, s=0):
    """What the reference reactor reports for segment s (one connection's stream): the complete
    messages in descriptor order — the fields of tests/golden/reassemble_ctl.json."""
    ob = regions[s][0]
    img = region_image(regions[s], seg_len[s])
    lens, parts = [], []
    for (o, n, _first, _nf, complete, _cont) in msgs[s]:
        if complete:
            lens.append(int(n))
            parts.append(img[int(o) - ob:int(o) - ob + int(n)])
    st = int(res[s]["status"])
    nf = int(res[s]["n_frames"]) - (1 if st in (-1, -4) else 0)
    return (lens, np.concatenate(parts) if parts else np.zeros(0, np.uint8), int(res[s]["consumed"]), nf,
            7 if st == -4 else 0, int(open_out[s]), int(cached_out[s]))
