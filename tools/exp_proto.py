"""The protocol check (websocketframeBatchCheckProtocolDevice) against a plain read of the same
descriptor bytes.

    python tools/exp_proto.py [--out profiles/proto_check.json] [--log2-frames 20]

One process, the bench protocol: 20 timed calls after 5, events at the two ends. Three shapes of
2^20 frames each (masked one-byte frames, messages of 16 fragments): (a) 2^20 segments of one
frame, (b) 2^16 segments of 16 frames, (c) one segment whose descriptors come from
websocketframeStreamDecodeDevice; each with and without d_frame_code, and each against
websocketframeGpuCalibrate mode 2 (read only, nontemporal loads) over as many bytes as the
descriptors take (32 B per frame). Writes the times and the ratios (check time / read time).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from util_amd import _lib  # noqa: E402
from util_amd import wsframe as W  # noqa: E402

WARM, TIMED = 5, 20
KEY = bytes([0x37, 0xFA, 0x21, 0x3D])


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


def frame(b0):
    return bytes([b0, 0x81]) + KEY + bytes([0x61 ^ KEY[0]])       # masked, one body byte: 7 bytes


def run(dev, name, nframes, per_seg, stream):
    """nframes frames in segments of per_seg (stream: one segment, decoded as a raw stream)"""
    unit = frame(0x81) if per_seg == 1 else frame(0x01) + frame(0x00) * 14 + frame(0x80)
    wire = torch.zeros(7 * nframes + W.BATCH_PAD, dtype=torch.uint8, device=dev)
    wire[:7 * nframes] = torch.from_numpy(np.frombuffer(unit, np.uint8).copy()).to(dev).repeat(7 * nframes // len(unit))
    nseg = 1 if stream else nframes // per_seg
    mf = nframes if stream else per_seg
    so = torch.arange(nseg, dtype=torch.int64, device=dev) * (7 * mf)
    sl = torch.full((nseg,), 7 * mf, dtype=torch.int64, device=dev)
    desc = torch.zeros(32 * nframes, dtype=torch.uint8, device=dev)
    res = torch.zeros(16 * nseg, dtype=torch.uint8, device=dev)
    if stream:
        W.stream_decode_device(wire, 7 * nframes, mf, desc, res)
    else:
        W.batch_decode_device(wire, so, sl, mf, desc, res)
    torch.cuda.synchronize()
    assert int(res.cpu().numpy().view(W.SEGRES_DTYPE)["n_frames"].sum()) == nframes, name
    pres = torch.zeros(16 * nseg, dtype=torch.uint8, device=dev)
    state = torch.zeros(nseg, dtype=torch.int64, device=dev)
    codes = torch.zeros(nframes, dtype=torch.uint8, device=dev)
    sink = torch.zeros(8, dtype=torch.uint8, device=dev)
    bench = _lib.load_bench_lib()
    st = torch.cuda.current_stream().cuda_stream

    def check(with_codes):
        W.batch_check_protocol_device(wire, so, desc, res, mf, pres, W.PROTO_EXPECT_MASKED, 0, 1 << 20, state,
                                      codes if with_codes else None)

    def read():
        _lib.check_bench(bench.websocketframeGpuCalibrate(desc.data_ptr(), sink.data_ptr(), 32 * nframes, 2, 1, 0, st),
                         "websocketframeGpuCalibrate")

    c_ms, n_ms, r_ms = timed(lambda: check(True)), timed(lambda: check(False)), timed(read)
    out = pres.cpu().numpy().view(W.PROTO_RES_DTYPE)
    assert (out["first_bad"] == W.PROTO_NONE).all() and (codes == 0).all() and (state == 0).all(), name
    return {"shape": name, "segments": nseg, "frames": nframes, "descriptor_bytes": 32 * nframes,
            "check_ms": round(c_ms, 4), "check_no_codes_ms": round(n_ms, 4), "read_ms": round(r_ms, 4),
            "check_over_read": round(c_ms / r_ms, 2), "check_no_codes_over_read": round(n_ms / r_ms, 2),
            "frames_per_us": round(nframes / (c_ms * 1e3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "proto_check.json"))
    ap.add_argument("--log2-frames", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = 1 << args.log2_frames
    results = [run(dev, "a: segments of 1 frame", n, 1, False), run(dev, "b: segments of 16 frames", n, 16, False),
               run(dev, "c: one segment, stream decode", n, 16, True)]
    doc = {"what": "websocketframeBatchCheckProtocolDevice vs websocketframeGpuCalibrate mode 2 (read only, nt loads) over "
                   "the descriptors' bytes; %d timed calls after %d, events at the two ends" % (TIMED, WARM),
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
