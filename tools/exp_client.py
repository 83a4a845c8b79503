"""The client handshake (websocketframeBatchClientVerifyDevice, websocketframeBatchClientRequestDevice)
against a plain read of the same bytes and against the server call at the same shape.

    python tools/exp_client.py [--out profiles/client_handshake.json] [--log2-big 20]

One process, the bench protocol: 20 timed calls after 5, events at the two ends. Shapes: 2^20 and
2^16 responses of about 200 bytes, 2^16 responses of 4 KiB (every response in a slot of its own
size rounded up to 16 bytes), and 2^20 requests with a 16-byte path. Each verify shape takes turns,
in the same process and on the same bytes, with websocketframeGpuCalibrate mode 2 (read only,
nontemporal loads) and with websocketframeBatchHandshakeDevice at the same nseg and segment size
(parse only: the server's parse kernel over the very same bytes, and over upgrade requests of the
same size, what it is built for). The request call is held against that accept-kernel time.
Three rounds of each, so the spread of the server call's own rounds is on record. After all GPU
timing the host entry is looped on one core. Prints the table of DESIGN 3.12.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import client_cases as CC  # noqa: E402
import client_oracle as CO  # noqa: E402
import handshake_cases as HC  # noqa: E402
from exp_handshake import browser_request, timed  # noqa: E402
from util_amd import _lib  # noqa: E402
from util_amd import wsframe as W  # noqa: E402

ROUNDS = 3


def server_response(size):
    """a response of `size` bytes: what a server sends, a Set-Cookie as the filler, one protocol"""
    head = [CC.STATUS_LINE, CC.UP, CC.CONN]
    tail = [CC.ACCEPT_NAME + CC.ACC, b"Sec-WebSocket-Protocol: chat"]
    room = size - len(CC.resp(head + [b"Set-Cookie: "] + tail))
    assert room >= 0
    return CC.resp(head + [b"Set-Cookie: " + CC.filler(room, 3)] + tail)


def plain_request(size):
    """an upgrade request of `size` bytes (a key, one protocol, a cookie as the filler)"""
    room = size - len(HC.request(proto=b"chat", before=b"Host: a\r\nCookie: \r\n"))
    assert room >= 0
    return HC.request(proto=b"chat", before=b"Host: a\r\nCookie: " + HC.filler(room, 3) + b"\r\n")


def tile(dev, one, nseg):
    size = len(one)
    stride = (size + 15) // 16 * 16
    row = np.zeros(stride, np.uint8)
    row[:size] = np.frombuffer(one, np.uint8)
    wire = torch.zeros(nseg * stride + W.BATCH_PAD, dtype=torch.uint8, device=dev)
    wire[:nseg * stride] = torch.from_numpy(row).to(dev).repeat(nseg)
    so = torch.arange(nseg, dtype=torch.int64, device=dev) * stride
    sl = torch.full((nseg,), size, dtype=torch.int64, device=dev)
    return wire, so, sl, stride


def spread(v):
    return {"min": round(min(v), 4), "max": round(max(v), 4), "median": round(sorted(v)[len(v) // 2], 4)}


def run_verify(dev, name, nseg, size):
    resp, reqs = server_response(size), plain_request(size)
    assert len(resp) == size == len(reqs)
    wire, so, sl, stride = tile(dev, resp, nseg)
    rwire, rso, rsl, _ = tile(dev, reqs, nseg)
    expect = torch.from_numpy(np.frombuffer(CC.EXPECT, np.uint8).copy()).to(dev).repeat(nseg)
    p, ent = CC.pool([(b"/", b"chat, superchat", b"")])
    strs = torch.from_numpy(p).to(dev)
    entry = torch.from_numpy(np.repeat(ent, nseg).view(np.uint8).reshape(-1).copy()).to(dev)
    cv = torch.zeros(32 * nseg, dtype=torch.uint8, device=dev)
    hs = torch.zeros(32 * nseg, dtype=torch.uint8, device=dev)
    sink = torch.zeros(8, dtype=torch.uint8, device=dev)
    bench = _lib.load_bench_lib()
    st = torch.cuda.current_stream().cuda_stream

    def verify():
        W.batch_client_verify_device(wire, so, sl, expect, cv, strs, entry)

    def server_parse_own():          # the server's parse kernel over the responses: same bytes, same shape
        W.batch_handshake_device(wire, so, sl, hs)

    def server_parse():              # ... and over requests of the same size, what it is built for
        W.batch_handshake_device(rwire, rso, rsl, hs)

    def read():
        _lib.check_bench(bench.websocketframeGpuCalibrate(wire.data_ptr(), sink.data_ptr(), nseg * stride, 2, 1, 0, st),
                         "websocketframeGpuCalibrate")

    t = {"verify": [], "server_parse_same_bytes": [], "server_parse_requests": [], "read": []}
    for _ in range(ROUNDS):
        for key, fn in (("verify", verify), ("read", read), ("server_parse_same_bytes", server_parse_own),
                        ("server_parse_requests", server_parse)):
            t[key].append(timed(fn))
    verify()
    torch.cuda.synchronize()
    want = CO.verify(resp, CC.EXPECT, b"chat, superchat")
    recs = cv.cpu().numpy().view(W.CLI_VERIFY_DTYPE)
    assert want[0] == size and all((recs[k] == want[i]).all() for i, k in enumerate(W.CLI_VERIFY_DTYPE.names)), name
    med = {k: spread(v)["median"] for k, v in t.items()}
    return {"shape": name, "responses": nseg, "response_bytes": size, "bytes": nseg * stride,
            "request_bytes_of_the_server_rows": len(reqs),
            "verify_ms": spread(t["verify"]), "read_ms": spread(t["read"]),
            "server_parse_same_bytes_ms": spread(t["server_parse_same_bytes"]),
            "server_parse_requests_ms": spread(t["server_parse_requests"]),
            "verify_over_read": round(med["verify"] / med["read"], 2),
            "verify_over_server_parse_same_bytes": round(med["verify"] / med["server_parse_same_bytes"], 2),
            "responses_per_us": round(nseg / (med["verify"] * 1e3), 2),
            "read_GBps": round(nseg * stride / (med["read"] * 1e6), 1)}


def run_request(dev, name, nseg):
    path = b"/chat/0123456789"
    assert len(path) == 16
    p, ent = CC.pool([(path, b"chat", b"")])
    strs = torch.from_numpy(p).to(dev)
    entry = torch.from_numpy(np.repeat(ent, nseg).view(np.uint8).reshape(-1).copy()).to(dev)
    nonce = torch.randint(0, 256, (16 * nseg,), dtype=torch.uint8, device=dev)
    cap = 192
    req = torch.zeros(cap * nseg, dtype=torch.uint8, device=dev)
    expect = torch.zeros(32 * nseg, dtype=torch.uint8, device=dev)
    rd = torch.zeros(16 * nseg, dtype=torch.uint8, device=dev)
    reqs = browser_request(500)
    rwire, rso, rsl, _ = tile(dev, reqs, nseg)
    hs = torch.zeros(32 * nseg, dtype=torch.uint8, device=dev)
    acc = torch.zeros(32 * nseg, dtype=torch.uint8, device=dev)
    resp = torch.zeros(160 * nseg, dtype=torch.uint8, device=dev)

    def request():
        W.batch_client_request_device(strs, entry, nonce, req, expect, rd, None, cap)

    def expect_only():
        W.batch_client_request_device(strs, entry, nonce, None, expect, rd, None, 0)

    def server_full():
        W.batch_handshake_device(rwire, rso, rsl, hs, W.HS_ECHO_PROTOCOL, acc, resp, None, 160)

    def server_parse():
        W.batch_handshake_device(rwire, rso, rsl, hs, W.HS_ECHO_PROTOCOL)

    t = {"request": [], "expect_only": [], "server_full": [], "server_parse": []}
    for _ in range(ROUNDS):
        for key, fn in (("request", request), ("server_full", server_full), ("expect_only", expect_only),
                        ("server_parse", server_parse)):
            t[key].append(timed(fn))
    request()
    torch.cuda.synchronize()
    nn = nonce.cpu().numpy().reshape(nseg, 16)
    r, e, d = req.cpu().numpy().reshape(nseg, cap), expect.cpu().numpy().reshape(nseg, 32), rd.cpu().numpy().view(W.CLI_REQ_DTYPE)
    for s in (0, 1, nseg // 2, nseg - 1):
        rec, text, exp = CO.request_record(path, bytes(nn[s]), b"chat", b"", cap)
        assert tuple(int(v) for v in d[s]) == rec and bytes(r[s][:len(text)]) == text and bytes(e[s]) == exp, (name, s)
    med = {k: spread(v)["median"] for k, v in t.items()}
    accept_ms = med["server_full"] - med["server_parse"]
    return {"shape": name, "requests": nseg, "path_bytes": 16, "request_bytes": int(d[0]["req_len"]),
            "request_ms": spread(t["request"]), "expect_only_ms": spread(t["expect_only"]),
            "server_call_ms": spread(t["server_full"]), "server_parse_ms": spread(t["server_parse"]),
            "server_accept_kernel_ms": round(accept_ms, 4), "request_over_server_accept": round(med["request"] / accept_ms, 2),
            "requests_per_us": round(nseg / (med["request"] * 1e3), 2)}


def cpu_side(size, n=1 << 14):
    """the host entries over n responses / requests, one core"""
    resp = server_response(size)
    t0 = time.perf_counter()
    for _ in range(n):
        W.client_verify_host(resp, CC.EXPECT, b"chat, superchat")
    dv = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(n):
        W.client_request_host(b"/chat/0123456789", CC.NONCE, b"chat")
    dr = time.perf_counter() - t0
    return {"response_bytes": size, "calls": n, "verify_one_core_us": round(dv / n * 1e6, 3),
            "request_one_core_us": round(dr / n * 1e6, 3),
            "note": "called through the Python wrappers: their buffer set-up (several us a call) is included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "client_handshake.json"))
    ap.add_argument("--log2-big", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    big = 1 << args.log2_big
    verify = [run_verify(dev, "a: 2^%d responses of 200 B" % args.log2_big, big, 200),
              run_verify(dev, "b: 2^16 responses of 200 B", 1 << 16, 200),
              run_verify(dev, "c: 2^16 responses of 4 KiB", 1 << 16, 4096)]
    request = [run_request(dev, "d: 2^%d requests, 16-byte path" % args.log2_big, big)]
    cpu = [cpu_side(200), cpu_side(4096)]
    doc = {"what": "websocketframeBatchClientVerifyDevice / RequestDevice vs websocketframeGpuCalibrate mode 2 (read only, nt "
                   "loads) and websocketframeBatchHandshakeDevice, taking turns; %d timed calls after %d, events at the two "
                   "ends, %d rounds each; identical bytes in every slot" % (20, 5, ROUNDS),
           "device": torch.cuda.get_device_name(0), "verify": verify, "request": request, "cpu": cpu}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    print("| shape | verify ms | read ms | server parse, same bytes ms | server parse, requests ms | verify / read | verify / server parse |")
    print("|---|---|---|---|---|---|---|")
    for r in verify:
        print("| %s | %.3f | %.3f | %.3f | %.3f | %.2f | %.2f |" % (
            r["shape"], r["verify_ms"]["median"], r["read_ms"]["median"], r["server_parse_same_bytes_ms"]["median"],
            r["server_parse_requests_ms"]["median"], r["verify_over_read"], r["verify_over_server_parse_same_bytes"]))
    for r in request:
        print("| %s | request %.3f ms | expect only %.3f ms | server accept kernel %.3f ms | ratio %.2f |" % (
            r["shape"], r["request_ms"]["median"], r["expect_only_ms"]["median"], r["server_accept_kernel_ms"],
            r["request_over_server_accept"]))


if __name__ == "__main__":
    main()
