"""The batch handshake (websocketframeBatchHandshakeDevice) against a plain read of the same bytes
and against the host symbols looped over the same requests.

    python tools/exp_handshake.py [--out profiles/handshake.json] [--log2-big 20]

One process, the bench protocol: 20 timed calls after 5, events at the two ends. Three shapes:
2^20 and 2^16 browser-like requests (about 500 bytes, a key of 24 characters, one protocol) and
2^16 requests of 4 KiB, every request in a slot of its own size rounded up to 16 bytes. Each shape:
the call with d_resp (echo mode), without d_resp (accept only) and parse only (neither: the parse
kernel alone, so the accept kernel is the difference), against websocketframeGpuCalibrate mode 2
(read only, nontemporal loads) over the same bytes. After all GPU timing, the reference's own
functions (oracle/_ref where present, else libwsframe_amd.so's host symbols) are looped over
2^14 of the requests on one core; the per-core rate times the granted cores is the CPU side.
Prints the table of DESIGN 3.9.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import handshake_cases as HC  # noqa: E402
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


def browser_request(size):
    """a request of `size` bytes: the headers a browser sends, a cookie as the filler"""
    head = (b"GET /chat HTTP/1.1\r\nHost: server.example.com\r\nConnection: Upgrade\r\nPragma: no-cache\r\n"
            b"Cache-Control: no-cache\r\nUpgrade: websocket\r\nOrigin: http://example.com\r\nSec-WebSocket-Version: 13\r\n"
            b"Accept-Encoding: gzip, deflate\r\nAccept-Language: en-US,en;q=0.9\r\n")
    tail = (b"Sec-WebSocket-Key: dGhlIHNhbXBsZSBub25jZQ==\r\nSec-WebSocket-Extensions: permessage-deflate\r\n"
            b"Sec-WebSocket-Protocol: chat\r\n\r\n")
    room = size - len(head) - len(tail) - len(b"Cookie: \r\n")
    return head + b"Cookie: " + HC.filler(room, 3) + b"\r\n" + tail


def run(dev, name, nseg, size):
    req = browser_request(size)
    assert len(req) == size
    stride = (size + 15) // 16 * 16
    one = np.zeros(stride, np.uint8)
    one[:size] = np.frombuffer(req, np.uint8)
    wire = torch.zeros(nseg * stride + W.BATCH_PAD, dtype=torch.uint8, device=dev)
    wire[:nseg * stride] = torch.from_numpy(one).to(dev).repeat(nseg)
    so = torch.arange(nseg, dtype=torch.int64, device=dev) * stride
    sl = torch.full((nseg,), size, dtype=torch.int64, device=dev)
    hs = torch.zeros(32 * nseg, dtype=torch.uint8, device=dev)
    acc = torch.zeros(32 * nseg, dtype=torch.uint8, device=dev)
    cap = 160
    resp = torch.zeros(cap * nseg, dtype=torch.uint8, device=dev)
    sink = torch.zeros(8, dtype=torch.uint8, device=dev)
    bench = _lib.load_bench_lib()
    st = torch.cuda.current_stream().cuda_stream

    def full():
        W.batch_handshake_device(wire, so, sl, hs, W.HS_ECHO_PROTOCOL, acc, resp, None, cap)

    def accept_only():
        W.batch_handshake_device(wire, so, sl, hs, W.HS_ECHO_PROTOCOL, acc)

    def parse_only():
        W.batch_handshake_device(wire, so, sl, hs, W.HS_ECHO_PROTOCOL)

    def read():
        _lib.check_bench(bench.websocketframeGpuCalibrate(wire.data_ptr(), sink.data_ptr(), nseg * stride, 2, 1, 0, st),
                         "websocketframeGpuCalibrate")

    f_ms, a_ms, p_ms, r_ms = timed(full), timed(accept_only), timed(parse_only), timed(read)
    full()
    torch.cuda.synchronize()
    x = HC.expected(HC.host_symbols(), req)
    recs = hs.cpu().numpy().view(W.HS_DTYPE)
    assert (recs["ret"] == x["ret"]).all() and (recs["flags"] == W.HS_RESP_WRITTEN).all(), name
    r = resp.cpu().numpy().reshape(nseg, cap)
    want = np.frombuffer(x["resp_echo"], np.uint8)
    assert (r[:, :len(want)] == want).all(), name
    return {"shape": name, "requests": nseg, "request_bytes": size, "bytes": nseg * stride,
            "call_ms": round(f_ms, 4), "call_no_resp_ms": round(a_ms, 4), "parse_kernel_ms": round(p_ms, 4),
            "accept_kernel_ms": round(f_ms - p_ms, 4), "read_ms": round(r_ms, 4),
            "call_over_read": round(f_ms / r_ms, 2), "call_no_resp_over_read": round(a_ms / r_ms, 2),
            "parse_over_read": round(p_ms / r_ms, 2), "requests_per_us": round(nseg / (f_ms * 1e3), 2),
            "read_GBps": round(nseg * stride / (r_ms * 1e6), 1)}


def cpu_side(size, n=1 << 14):
    """the reference's functions (or the host symbols) over n requests, one core"""
    lib = HC.reference_lib()
    which = "oracle/_ref/libwsref.so"
    if lib is None:
        lib, which = HC.host_symbols(), "libwsframe_amd.so host symbols"
    req = browser_request(size)
    buf = C.create_string_buffer(req, len(req))
    base = C.addressof(buf)
    sk, skl, sp, spl = C.c_void_p(0), C.c_uint(0), C.c_void_p(0), C.c_uint(0)
    acc = C.create_string_buffer(60)
    t0 = time.perf_counter()
    for _ in range(n):
        lib.websocketframeDecodeHandshakeRequest(base, len(req), C.byref(sk), C.byref(skl), C.byref(sp), C.byref(spl))
        lib.websocketframeComputeSecAccept(sk.value, skl.value, acc)
        lib.websocketframeFreeString(lib.websocketframeEncodeHandshakeResponseWithProtocol(acc, 28, sp.value, spl.value))
    dt = time.perf_counter() - t0
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    cores = min(cores, int(os.environ.get("OMP_NUM_THREADS", cores)))
    return {"library": which, "request_bytes": size, "requests": n, "one_core_us_per_request": round(dt / n * 1e6, 3),
            "cores": cores, "projected_requests_per_us_all_cores": round(cores * n / (dt * 1e6), 2),
            "note": "called through ctypes: the per-call glue (about 1 us for three calls) is included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "handshake.json"))
    ap.add_argument("--log2-big", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    results = [run(dev, "a: 2^%d requests of 500 B" % args.log2_big, 1 << args.log2_big, 500),
               run(dev, "b: 2^16 requests of 500 B", 1 << 16, 500), run(dev, "c: 2^16 requests of 4 KiB", 1 << 16, 4096)]
    cpu = [cpu_side(500), cpu_side(4096)]
    doc = {"what": "websocketframeBatchHandshakeDevice vs websocketframeGpuCalibrate mode 2 (read only, nt loads) over the "
                   "same bytes; %d timed calls after %d, events at the two ends; identical requests in every slot" % (TIMED, WARM),
           "device": torch.cuda.get_device_name(0), "results": results, "cpu": cpu}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    print("| shape | call ms | no resp ms | parse ms | accept ms | read ms | call / read | requests / us |")
    print("|---|---|---|---|---|---|---|---|")
    for r in results:
        print("| %s | %.3f | %.3f | %.3f | %.3f | %.3f | %.2f | %.1f |" % (
            r["shape"], r["call_ms"], r["call_no_resp_ms"], r["parse_kernel_ms"], r["accept_kernel_ms"], r["read_ms"],
            r["call_over_read"], r["requests_per_us"]))


if __name__ == "__main__":
    main()
