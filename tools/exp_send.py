"""The batch message send (websocketframeBatchSendDevice) against the batch encode
(websocketframeBatchEncodeDevice) over the identical frame list, and on fragmented and small shapes.

    python tools/exp_send.py [--out profiles/send.json] [--log2-msgs 20]

One process, the bench protocol: 20 timed calls after 5, events at the two ends.
  (a) 2^20 x 4 KiB messages (cfg2's bytes; 2^16 connections of 16), unfragmented, server and client
      role. The encode call over the same 2^20 frames is the yardstick: the two are timed in turn,
      ROUNDS times each, on two output buffers; both times, their spreads and the ratio are
      recorded, and the two outputs are compared byte for byte.
  (b) the same bytes with F = 1464 (the reference's inbuf size): 3 frames per message.
  (c) 2^20 connections x one 125-byte message.
  (d) 64 messages of 64 MiB, one per connection: every message's thread writes 4096 piece pointers.
Algorithmic bytes = body read + wire written; GB/s and the share of the 8 TB/s HBM peak from them.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from util_amd import wsframe as W  # noqa: E402

WARM, TIMED, ROUNDS = 5, 20, 4
PEAK = 8000.0   # GB/s


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(TIMED):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / TIMED


def up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def rates(ms, nbytes):
    gbs = nbytes / (ms * 1e6)
    return {"ms": round(ms, 4), "GB_per_s": round(gbs, 1), "hbm_frac": round(gbs / PEAK, 4)}


class Send:
    def __init__(self, dev, src, nseg, mm, length, stride, F, client):
        n = nseg * mm
        msg = np.zeros(n, W.SEND_MSG_DTYPE)
        msg["src_off"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
        msg["len"], msg["type"] = length, 2
        self.src, self.mm, self.n = src, mm, n
        self.msg = up(dev, msg)
        self.nmsg = torch.full((nseg,), mm, dtype=torch.int32, device=dev)
        self.frag = None if F is None else torch.full((nseg,), F, dtype=torch.int32, device=dev)
        self.keys_np = (np.arange(1, n + 1, dtype=np.uint64) * 0x9E3779B1 % (1 << 32)).astype(np.uint32) if client else None
        self.keys = None if not client else up(dev, self.keys_np).view(torch.int32)
        self.off = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
        self.res = torch.zeros(32 * nseg, dtype=torch.uint8, device=dev)
        self.tx = None
        self.call(0)
        torch.cuda.synchronize()
        self.total = int(self.off[-1].item())
        r = self.res.cpu().numpy().view(W.SEND_RES_DTYPE)
        assert not r["status"].any()
        self.frames = int(r["n_frames"].sum())
        self.tx = torch.zeros(self.total + 64, dtype=torch.uint8, device=dev)
        self.bytes = n * length + self.total

    def call(self, cap=None):
        W.batch_send_device(self.src, self.msg, self.nmsg, self.mm, self.tx, self.off, self.res, frag_size=self.frag,
                            mask_key=self.keys, tx_capacity=self.total if cap is None else cap)


def shape_a(dev, src, log2, client):
    n = 1 << log2
    s = Send(dev, src, n // 16, 16, 4096, 4096, None, client)
    fr = np.zeros(n, W.ENC_DTYPE)
    fr["src_off"] = np.arange(n, dtype=np.uint64) * np.uint64(4096)
    fr["len"], fr["type"], fr["is_fin"], fr["prev_is_fin"] = 4096, 2, 1, 1
    if client:
        fr["masked"], fr["mask_key"] = 1, s.keys_np
    frames = up(dev, fr)
    dst = torch.zeros(s.total + 64, dtype=torch.uint8, device=dev)
    woff = torch.zeros(n + 1, dtype=torch.int64, device=dev)

    def enc():
        W.batch_encode_device(src, frames, dst, woff, capacity=s.total)
    send_ms, enc_ms = [], []
    for _ in range(ROUNDS):
        send_ms.append(timed(s.call))
        enc_ms.append(timed(enc))
    torch.cuda.synchronize()
    assert int(woff[-1].item()) == s.total and torch.equal(dst[:s.total], s.tx[:s.total]), "send and encode differ"
    sm, em = float(np.mean(send_ms)), float(np.mean(enc_ms))
    return {"shape": "a: 2^%d x 4 KiB unfragmented, %s role" % (log2, "client" if client else "server"), "messages": n,
            "frames": s.frames, "algorithmic_bytes": s.bytes, "send": rates(sm, s.bytes), "encode": rates(em, s.bytes),
            "send_ms_rounds": [round(v, 4) for v in send_ms], "encode_ms_rounds": [round(v, 4) for v in enc_ms],
            "encode_spread": round(max(enc_ms) / min(enc_ms), 4), "send_spread": round(max(send_ms) / min(send_ms), 4),
            "send_over_encode": round(sm / em, 4), "send_capacity0_ms": round(timed(lambda: s.call(0)), 4),
            "outputs_equal": True}


def shape_plain(dev, src, name, nseg, mm, length, stride, F, client):
    s = Send(dev, src, nseg, mm, length, stride, F, client)
    ms = [timed(s.call) for _ in range(2)]
    return {"shape": "%s, %s role" % (name, "client" if client else "server"), "messages": s.n, "frames": s.frames,
            "algorithmic_bytes": s.bytes, "send": rates(float(np.mean(ms)), s.bytes), "send_ms_rounds": [round(v, 4) for v in ms],
            "send_capacity0_ms": round(timed(lambda: s.call(0)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "send.json"))
    ap.add_argument("--log2-msgs", type=int, default=20)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    k = args.log2_msgs
    n = 1 << k
    src = torch.empty(n * 4096, dtype=torch.uint8, device=dev)
    step = 1 << 28
    for a in range(0, src.numel(), step):
        src[a:a + step] = torch.randint(0, 256, (min(step, src.numel() - a),), dtype=torch.uint8, device=dev)
    results = []
    for client in (False, True):
        if "a" in (args.only or "a"):
            results.append(shape_a(dev, src, k, client))
        if "b" in (args.only or "b"):
            results.append(shape_plain(dev, src, "b: 2^%d x 4 KiB, F = 1464" % k, n // 16, 16, 4096, 4096, 1464, client))
        if "c" in (args.only or "c"):
            results.append(shape_plain(dev, src, "c: 2^%d connections x one 125-byte message" % k, n, 1, 125, 128, None, client))
        if "d" in (args.only or "d") and k >= 14:
            big = n * 4096 // 64
            results.append(shape_plain(dev, src, "d: 64 connections x one %d MiB message" % (big >> 20), 64, 1, big, big, None, client))
    doc = {"what": "websocketframeBatchSendDevice; (a) against websocketframeBatchEncodeDevice over the identical frame list, "
                   "timed in turn %d times each on two output buffers; %d timed calls after %d, events at the two ends; "
                   "algorithmic bytes = body read + wire written, hbm_frac against %d GB/s" % (ROUNDS, TIMED, WARM, int(PEAK)),
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
