"""The control replies (websocketframeBatchControlRepliesDevice) against a plain read of the same
descriptors and ping bodies, and against the host loop they replace.

    python tools/exp_reply.py [--out profiles/reply.json] [--log2-frames 20]

One process, the bench protocol: 20 timed calls after 5, events at the two ends. The shapes of
tools/exp_proto.py, 2^20 masked one-byte frames each and no ping among them (the cost of finding
out that there is nothing to say): (a) 2^20 segments of one frame, (b) 2^16 segments of 16 frames,
(c) one segment whose descriptors come from websocketframeStreamDecodeDevice; and (d) 2^16 segments
of 16 frames of which one is a PING with 16 body bytes. Each against
  - websocketframeGpuCalibrate mode 2 (read only, nontemporal loads) over as many bytes as the
    descriptors (32 B per frame) and the ping bodies take: the floor;
  - the same call with tx_capacity 0 (every pass runs, no reply byte is stored);
  - websocketframeControlRepliesHost looped over the segments by 16 threads (tools/reply_host_loop.c:
    a length pass, a prefix sum, a write pass), descriptors and wire already in host memory: what
    the call replaces, without the copies to the host that path also needs.
Writes the times and the ratios (call / read, host loop / call).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from util_amd import _lib  # noqa: E402
from util_amd import wsframe as W  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
WARM, TIMED, THREADS = 5, 20, 16
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


def frame(b0, body=b"a"):
    return bytes([b0, 0x80 | len(body)]) + KEY + bytes(b ^ KEY[i & 3] for i, b in enumerate(body))


def host_loop_lib(tmp):
    so = os.path.join(tmp, "libreply_host_loop.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-pthread", os.path.join(HERE, "reply_host_loop.c"), "-o", so,
                    "-L" + _lib.HERE, "-l:libwsframe_amd_reply.so", "-Wl,-rpath," + _lib.HERE], check=True)
    _lib.load_reply_lib()
    lib = C.CDLL(so)
    vp, u32 = C.c_void_p, C.c_uint
    lib.reply_host_loop.restype = C.c_longlong
    lib.reply_host_loop.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, C.c_int]
    return lib


def run(dev, host, name, nframes, per_seg, stream, ping):
    """nframes frames in segments of per_seg (stream: one segment, decoded as a raw stream); ping:
    frame 5 of every 16 is a PING with 16 body bytes"""
    if per_seg == 1:
        unit = frame(0x81)
    else:
        unit = b"".join(frame(0x89, b"0123456789abcdef") if ping and i == 5 else frame(0x01 if i == 0 else (0x80 if i == 15 else 0x00))
                        for i in range(16))
    reps = nframes // (1 if per_seg == 1 else 16)
    nbytes = len(unit) * reps
    wire = torch.zeros(nbytes + W.BATCH_PAD, dtype=torch.uint8, device=dev)
    wire[:nbytes] = torch.from_numpy(np.frombuffer(unit, np.uint8).copy()).to(dev).repeat(reps)
    nseg = 1 if stream else nframes // per_seg
    mf = nframes if stream else per_seg
    seg_bytes = nbytes // nseg
    so = torch.arange(nseg, dtype=torch.int64, device=dev) * seg_bytes
    sl = torch.full((nseg,), seg_bytes, dtype=torch.int64, device=dev)
    desc = torch.zeros(32 * nframes, dtype=torch.uint8, device=dev)
    res = torch.zeros(16 * nseg, dtype=torch.uint8, device=dev)
    if stream:
        W.stream_decode_device(wire, nbytes, mf, desc, res)
    else:
        W.batch_decode_device(wire, so, sl, mf, desc, res)
    torch.cuda.synchronize()
    assert int(res.cpu().numpy().view(W.SEGRES_DTYPE)["n_frames"].sum()) == nframes, name
    npings = reps if ping else 0
    total = 18 * npings
    tx = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    off = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
    rres = torch.zeros(16 * nseg, dtype=torch.uint8, device=dev)
    sink = torch.zeros(8, dtype=torch.uint8, device=dev)
    bench = _lib.load_bench_lib()
    st = torch.cuda.current_stream().cuda_stream
    read_bytes = 32 * nframes + 16 * npings

    def call(cap=None):
        W.batch_control_replies_device(wire, so, desc, res, mf, tx, off, rres, tx_capacity=cap)

    def read():
        _lib.check_bench(bench.websocketframeGpuCalibrate(desc.data_ptr(), sink.data_ptr(), 32 * nframes, 2, 1, 0, st),
                         "websocketframeGpuCalibrate")
        if npings:
            _lib.check_bench(bench.websocketframeGpuCalibrate(wire.data_ptr(), sink.data_ptr(), 16 * npings, 2, 1, 0, st),
                             "websocketframeGpuCalibrate")

    c_ms, z_ms, r_ms = timed(call), timed(lambda: call(0)), timed(read)
    call()
    torch.cuda.synchronize()
    g_off, g_tx, g_res = off.cpu().numpy().view(np.uint64), tx.cpu().numpy(), rres.cpu().numpy().view(W.REPLY_RES_DTYPE)
    assert int(g_off[-1]) == total and int(g_res["n_pong"].sum()) == npings, name
    # the host loop on the same descriptors and (decoded) wire, already in host memory
    h_wire, h_so, h_desc, h_res = wire.cpu().numpy(), so.cpu().numpy().view(np.uint64), desc.cpu().numpy(), res.cpu().numpy()
    h_tx, h_off, h_out = np.zeros(total + 64, np.uint8), np.zeros(nseg + 1, np.uint64), np.zeros(nseg, W.REPLY_RES_DTYPE)

    def loop():
        n = host.reply_host_loop(h_wire.ctypes.data, h_so.ctypes.data, h_desc.ctypes.data, h_res.ctypes.data, nseg, mf, 0,
                                 h_tx.ctypes.data, h_off.ctypes.data, h_out.ctypes.data, THREADS)
        assert n == total, name

    loop()
    t0 = time.perf_counter()
    for _ in range(3):
        loop()
    h_ms = (time.perf_counter() - t0) / 3 * 1e3
    assert np.array_equal(h_off, g_off) and np.array_equal(h_tx[:total], g_tx[:total]) and np.array_equal(h_out, g_res), name
    return {"shape": name, "segments": nseg, "frames": nframes, "pings": npings, "reply_bytes": total, "read_bytes": read_bytes,
            "call_ms": round(c_ms, 4), "call_capacity0_ms": round(z_ms, 4), "read_ms": round(r_ms, 4),
            "host_loop_ms": round(h_ms, 3), "host_threads": THREADS, "call_over_read": round(c_ms / r_ms, 2),
            "host_loop_over_call": round(h_ms / c_ms, 1), "frames_per_us": round(nframes / (c_ms * 1e3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "reply.json"))
    ap.add_argument("--log2-frames", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = 1 << args.log2_frames
    with tempfile.TemporaryDirectory() as tmp:
        host = host_loop_lib(tmp)
        results = [run(dev, host, "a: segments of 1 frame", n, 1, False, False),
                   run(dev, host, "b: segments of 16 frames", n, 16, False, False),
                   run(dev, host, "c: one segment, stream decode", n, 16, True, False),
                   run(dev, host, "d: segments of 16 frames, 1 ping per 16", n, 16, False, True)]
    doc = {"what": "websocketframeBatchControlRepliesDevice vs websocketframeGpuCalibrate mode 2 (read only, nt loads) over the "
                   "descriptors' and ping bodies' bytes, and vs websocketframeControlRepliesHost looped over the segments by "
                   "%d threads; %d timed calls after %d, events at the two ends (host loop: 3 timed runs after 1, host clock)"
                   % (THREADS, TIMED, WARM),
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
