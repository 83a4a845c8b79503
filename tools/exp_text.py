"""The text validator (websocketframeBatchValidateTextDevice) against a plain read of the same bytes.

    python tools/exp_text.py [--out profiles/text_validate.json] [--nseg 262144] [--big-mib 256]

One process, the bench protocol: 20 timed calls after 5, events at the two ends. Three workloads:
(a) cfg5-shaped reassembly output (one 16 KiB message per 16-slot segment), all ASCII;
(b) the same bytes as mixed 1- to 4-byte sequences; (c) one message of --big-mib MiB. Each is
timed against websocketframeGpuCalibrate mode 2 (read only, nontemporal loads) over the same
number of bytes of the same buffer. Writes the ratios (validator time / read time) and GiB/s.
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


def mixed_block(n):
    """n bytes of well-formed text, code points of all four lengths in equal shares"""
    rng = np.random.default_rng(5)
    lo = np.array([0x20, 0x80, 0x800, 0x10000])[rng.integers(0, 4, n)]
    hi = np.array([0x7F, 0x800, 0xD800, 0x110000])[np.searchsorted([0x20, 0x80, 0x800, 0x10000], lo)]
    cp = (lo + (rng.random(n) * (hi - lo)).astype(np.int64)).astype("<u4")
    b = cp.tobytes().decode("utf-32-le").encode("utf-8")[:n]
    while True:
        try:
            b.decode("utf-8")
            break
        except UnicodeDecodeError:
            b = b[:-1]
    return np.frombuffer(b + b"." * (n - len(b)), np.uint8).copy()


def run(dev, name, nseg, mf, body, stride, block):
    """nseg segments of one complete text message of `body` bytes each, `stride` bytes apart,
    every body a copy of block[:body]"""
    out = torch.zeros(nseg * stride + 64, dtype=torch.uint8, device=dev)
    rows = out[:nseg * stride].view(nseg, stride)
    rows[:, :body] = torch.from_numpy(block[:body]).to(dev)
    msg = np.zeros(nseg * mf, dtype=W.MSG_DTYPE)
    desc = np.zeros(nseg * mf, dtype=W.DESC_DTYPE)
    first = np.arange(nseg) * mf
    msg["out_off"][first] = np.arange(nseg, dtype=np.uint64) * np.uint64(stride)
    msg["len"][first] = body
    msg["n_frames"][first] = mf
    msg["complete"][first] = 1
    desc["type"][first] = 1
    d_msg, d_desc = torch.from_numpy(msg.view(np.uint8)).to(dev), torch.from_numpy(desc.view(np.uint8)).to(dev)
    nmsg = torch.ones(nseg, dtype=torch.int32, device=dev)
    verdict = torch.zeros(nseg * mf, dtype=torch.int32, device=dev)
    first_bad = torch.zeros(nseg, dtype=torch.int32, device=dev)
    state = torch.zeros(nseg, dtype=torch.int32, device=dev)
    sink = torch.zeros(8, dtype=torch.uint8, device=dev)
    nbytes = nseg * body
    bench = _lib.load_bench_lib()
    st = torch.cuda.current_stream().cuda_stream

    def validate():
        W.batch_validate_text_device(out, d_desc, d_msg, nmsg, mf, verdict, text_state=state, first_bad=first_bad)

    def read():
        _lib.check_bench(bench.websocketframeGpuCalibrate(out.data_ptr(), sink.data_ptr(), nbytes // 16 * 16, 2, 1, 0, st),
                         "websocketframeGpuCalibrate")

    v_ms, r_ms = timed(validate), timed(read)
    v = verdict.cpu().numpy()[first]
    assert (v == W.TEXT_VALID).all() and (first_bad.cpu().numpy().view(np.uint32) == W.TEXT_NONE).all(), name
    gib = nbytes / 2.0 ** 30
    return {"workload": name, "messages": nseg, "body_bytes": body, "checked_bytes": nbytes,
            "validate_ms": round(v_ms, 4), "validate_GiBps": round(gib / (v_ms / 1e3), 1),
            "read_ms": round(r_ms, 4), "read_GiBps": round(gib / (r_ms / 1e3), 1),
            "validate_over_read": round(v_ms / r_ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "text_validate.json"))
    ap.add_argument("--nseg", type=int, default=1 << 18)
    ap.add_argument("--big-mib", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    body, stride = 16 * 1024, 16 * 1032                       # cfg5: 16 fragments of 1 KiB, 8-B headers
    big = args.big_mib << 20
    results = [
        run(dev, "a: cfg5 shape, ASCII", args.nseg, 16, body, stride, np.full(body, 0x61, np.uint8)),
        run(dev, "b: cfg5 shape, mixed 1-4-byte sequences", args.nseg, 16, body, stride, mixed_block(body)),
        run(dev, "c: one message", 1, 1, big, big, np.tile(mixed_block(1 << 20), args.big_mib)),
    ]
    doc = {"what": "websocketframeBatchValidateTextDevice vs websocketframeGpuCalibrate mode 2 (read only, nt loads) "
                   "over the same bytes of the same buffer; %d timed calls after %d, events at the two ends" % (TIMED, WARM),
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
