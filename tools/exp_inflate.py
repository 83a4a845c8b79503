"""websocketframeBatchInflateDevice on four workloads -> profiles/inflate.json.

    python tools/exp_inflate.py [--out profiles/inflate.json] [--only a,b,c,d]

20 timed calls after 5 (events, median), per workload: compressed and inflated bytes, time, inflated
GiB/s, the ratio to websocketframeGpuCalibrate's copy moving the same number of bytes (compressed +
inflated), and the ratios to the host rule (util_amd/csrc/ws_inflate.h) and to zlib's own inflate on
16 threads (a helper compiled here with g++ and linked to libz; the host side runs a share of the
connections and is compared by throughput). The outputs of the first call are checked against zlib.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from util_amd import _lib  # noqa: E402
from util_amd import wsframe as W  # noqa: E402

HELPER = r"""
#include <chrono>
#include <thread>
#include <vector>
#include <string.h>
#include <zlib.h>
#include "util_amd/csrc/ws_inflate.h"
// messages [0, n): body src + off[i], len[i] -> dst + out[i]; which: 0 the host rule, 1 zlib. Seconds.
extern "C" double run(int which, const unsigned char* src, const unsigned long long* off, const unsigned long long* len,
                      const unsigned long long* out, unsigned long long n, int threads, unsigned char* dst,
                      unsigned long long* bad) {
    std::vector<std::thread> th;
    std::vector<unsigned long long> fails(threads, 0);
    const auto t0 = std::chrono::steady_clock::now();
    for (int t = 0; t < threads; ++t)
        th.emplace_back([=, &fails] {
            const unsigned long long lo = n * t / threads, hi = n * (t + 1) / threads;
            z_stream z;
            memset(&z, 0, sizeof(z));
            if (which) inflateInit2(&z, -15);
            static const unsigned char tail[4] = {0, 0, 0xFF, 0xFF};
            for (unsigned long long i = lo; i < hi; ++i) {
                const unsigned long long room = out[i + 1] - out[i];
                if (which) {
                    inflateReset(&z);
                    z.next_in = const_cast<unsigned char*>(src + off[i]);
                    z.avail_in = (unsigned)len[i];
                    z.next_out = dst + out[i];
                    z.avail_out = (unsigned)room;
                    int rc = inflate(&z, Z_SYNC_FLUSH);
                    z.next_in = const_cast<unsigned char*>(tail);
                    z.avail_in = 4;
                    if (rc == Z_OK || rc == Z_BUF_ERROR) rc = inflate(&z, Z_SYNC_FLUSH);
                    if ((rc != Z_OK && rc != Z_BUF_ERROR && rc != Z_STREAM_END) || z.avail_out) ++fails[t];
                } else {
                    WebsocketInflateMsg_t m = {off[i], len[i], WEBSOCKET_INFLATE_RAW, 0};
                    WebsocketInflateResult_t r;
                    ws_inflate_connection(src, off[i] + len[i], &m, 1, 0, dst + out[i], room, 0, &r);
                    if (r.status || r.out_len != room) ++fails[t];
                }
            }
            if (which) inflateEnd(&z);
        });
    for (auto& x : th) x.join();
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *bad = 0;
    for (auto f : fails) *bad += f;
    return s;
}
"""


def build_helper(tmp):
    src, so = os.path.join(tmp, "inflate_cmp.cpp"), os.path.join(tmp, "libinflate_cmp.so")
    open(src, "w").write(HELPER)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-I", REPO, src, "-lz", "-o", so], check=True)
    lib = C.CDLL(so)
    lib.run.restype = C.c_double
    lib.run.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_ulonglong, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def deflate(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    return (c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH))[:-4]


def json_like(rng, n):
    """about n bytes of JSON-like text"""
    keys = ["id", "user", "name", "timestamp", "status", "payload", "items", "price", "active", "channel", "seq", "tags"]
    parts = []
    size = 0
    while size < n:
        k = keys[int(rng.integers(0, len(keys)))]
        u = rng.random()
        v = str(int(rng.integers(0, 1 << 31))) if u < 0.4 else ('"%s"' % "".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(rng.integers(3, 14)))) if u < 0.8 else "true")
        p = '"%s": %s, ' % (k, v)
        parts.append(p)
        size += len(p)
    return ("{" + "".join(parts))[:n - 1].encode() + b"}"


def long_text(rng, n):
    base = json_like(rng, 1 << 18)
    parts, size = [], 0
    while size < n:
        o, ln = int(rng.integers(0, len(base) - 4096)), int(rng.integers(100, 4096))
        parts.append(base[o:o + ln])
        size += ln
    return b"".join(parts)[:n]


def workload(name, rng):
    """(pool of bodies, pool of plain texts, connections, messages per connection)"""
    if name == "a":
        plain = [json_like(rng, 1024) for _ in range(512)]
        return [deflate(p, 6) for p in plain], plain, 256 * 1024, 1
    if name in ("b", "c"):
        plain = [json_like(rng, 16384) for _ in range(64)]
        return [deflate(p, 6 if name == "b" else 0) for p in plain], plain, 64 * 1024, 4
    plain = [long_text(rng, 16 << 20)]
    return [deflate(plain[0], 6)], plain, 64, 1


def run(name, dev, helper, bench):
    rng = np.random.default_rng(ord(name))
    pool, plain, nconn, mm = workload(name, rng)
    npool, nmsg_all = len(pool), nconn * mm
    idx = np.arange(nmsg_all) % npool
    plen = np.array([len(b) for b in pool], np.uint64)
    olen = np.array([len(p) for p in plain], np.uint64)
    # every message has its own copy of its body: the source is the pool tiled
    poolsrc = np.frombuffer(b"".join(pool), np.uint8)
    poff = np.concatenate([[0], np.cumsum(plen)]).astype(np.uint64)
    reps = (nmsg_all + npool - 1) // npool
    src = torch.from_numpy(poolsrc.copy()).to(dev).repeat(reps)
    off = (np.arange(nmsg_all, dtype=np.uint64) // np.uint64(npool)) * np.uint64(len(poolsrc)) + poff[idx]
    msg = np.zeros(nmsg_all, W.INFLATE_MSG_DTYPE)
    msg["src_off"], msg["len"], msg["kind"] = off, plen[idx], W.INFLATE_RAW
    outs = olen[idx]
    out_off = np.concatenate([[0], np.cumsum(outs)]).astype(np.uint64)
    caps = outs.reshape(nconn, mm).sum(1)
    doff = out_off[:-1].reshape(nconn, mm)[:, 0].copy()
    comp, inf = int(plen[idx].sum()), int(outs.sum())
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    d_msg, d_nmsg = T(msg), torch.full((nconn,), mm, dtype=torch.int32, device=dev)
    d_off, d_cap = T(doff).view(torch.int64), T(caps).view(torch.int64)
    dst = torch.zeros(inf + 64, dtype=torch.uint8, device=dev)
    mres = torch.zeros(24 * nmsg_all, dtype=torch.uint8, device=dev)
    res = torch.zeros(24 * nconn, dtype=torch.uint8, device=dev)

    def call():
        W.batch_inflate_device(src, d_msg, d_nmsg, mm, dst, d_off, d_cap, mres, res)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    first = timed(call)
    r = res.cpu().numpy().view(W.INFLATE_RES_DTYPE)
    assert not r["status"].any() and int(r["out_len"].sum()) == inf, "the device call failed on workload " + name
    for k in sorted({0, nmsg_all // 3, nmsg_all - 1}):
        o, n = int(out_off[k]), int(outs[k])
        assert dst[o:o + n].cpu().numpy().tobytes() == plain[int(idx[k])], "wrong output on workload " + name
    warm, iters = (5, 20) if first < 1500 else (1, 5)
    for _ in range(warm - 1):
        call()
    ts = sorted(timed(call) for _ in range(iters))
    ms = ts[len(ts) // 2]
    # the copy that moves as many bytes: (compressed + inflated) / 2 read and as many written
    ncopy = min((comp + inf) // 2 // 16 * 16, dst.numel() // 16 * 16)
    scratch = torch.empty(ncopy, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def copy():
        assert bench.websocketframeGpuCalibrate(dst.data_ptr(), scratch.data_ptr(), ncopy, 1, 1, 0, st) == 0
    for _ in range(5):
        copy()
    cs = sorted(timed(copy) for _ in range(20))
    copy_ms = cs[10] * ((comp + inf) / 2 / ncopy)
    del scratch
    # the host: a share of the messages (at most 512 MiB of output), 16 threads, best of 3, by throughput
    share = nmsg_all
    while share > 16 and int(out_off[share]) > (512 << 20):
        share //= 2
    hsrc = np.tile(poolsrc, (share + npool - 1) // npool)
    hdst = np.zeros(int(out_off[share]) + 64, np.uint8)
    a_off, a_len, a_out = off[:share].copy(), plen[idx][:share].copy(), out_off[:share + 1].copy()
    host = {}
    for which, label in ((0, "host_rule"), (1, "zlib")):
        best = None
        for _ in range(3):
            bad = C.c_ulonglong(0)
            s = helper.run(which, hsrc.ctypes.data, a_off.ctypes.data, a_len.ctypes.data, a_out.ctypes.data, share, 16,
                           hdst.ctypes.data, C.byref(bad))
            assert bad.value == 0, label
            best = s if best is None else min(best, s)
        host[label] = int(out_off[share]) / best / 2**30
    gibs = inf / (ms / 1e3) / 2**30
    return {"workload": name, "connections": nconn, "messages_per_connection": mm, "compressed_bytes": comp,
            "inflated_bytes": inf, "first_call_ms": round(first, 3), "timed_calls": iters, "warm_calls": warm,
            "median_ms": round(ms, 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4),
            "inflated_GiBps": round(gibs, 3), "copy_same_bytes_ms": round(copy_ms, 4),
            "ratio_to_copy": round(copy_ms / ms, 4), "host_share_messages": share, "host_threads": 16,
            "host_rule_GiBps": round(host["host_rule"], 3), "zlib_GiBps": round(host["zlib"], 3),
            "ratio_to_host_rule": round(gibs / host["host_rule"], 3), "ratio_to_zlib": round(gibs / host["zlib"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "inflate.json"))
    ap.add_argument("--only", default="a,b,c,d")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    bench = _lib.load_bench_lib()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        helper = build_helper(tmp)
        for name in args.only.split(","):
            rows.append(run(name, dev, helper, bench))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    doc = {"tool": "tools/exp_inflate.py", "device": torch.cuda.get_device_name(0),
           "method": "median of the timed calls after the warm calls, HIP events around each call; host: 16 threads, best of 3, "
                     "a share of the messages, compared by inflated GiB/s",
           "workloads": {"a": "256 Ki connections x one 1 KiB JSON-like message, level 6",
                         "b": "64 Ki connections x 4 messages of 16 KiB, level 6",
                         "c": "as b, level 0 (stored blocks)", "d": "64 connections x one 16 MiB message, level 6"},
           "rows": rows}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
