"""websocketframeBatchDeflateDevice on four workloads -> profiles/deflate.json.

    python tools/exp_deflate.py [--out profiles/deflate.json] [--only a,b,c,d]

20 timed calls after 5 (events, median), per workload: input and output bytes, time, input GiB/s,
the output next to zlib level 1 and level 1 Z_FIXED on the same messages, the ratio to
websocketframeGpuCalibrate's copy moving the same number of bytes (input + output), and the ratio to
zlib level 1 on 16 threads (a helper compiled here with g++ and linked to libz; the host side runs a
share of the messages and is compared by throughput). Rooms of the first call are checked with zlib.
The sizes on tests/inflate_cases.text(seed 1) at 1, 4 and 16 KiB are recorded too.
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
sys.path.insert(0, os.path.join(REPO, "tools"))
from util_amd import _lib  # noqa: E402
from util_amd import wsframe as W  # noqa: E402
from exp_inflate import json_like, long_text  # noqa: E402

HELPER = r"""
#include <chrono>
#include <thread>
#include <vector>
#include <string.h>
#include <zlib.h>
// messages [0, n): body src + off[i], len[i], compressed by zlib level 1 (raw, sync flush) into a
// per-thread buffer. Returns seconds; *total the compressed bytes (tails of 4 taken off).
extern "C" double run(const unsigned char* src, const unsigned long long* off, const unsigned long long* len,
                      unsigned long long n, int threads, unsigned long long* total) {
    std::vector<std::thread> th;
    std::vector<unsigned long long> sums(threads, 0);
    const auto t0 = std::chrono::steady_clock::now();
    for (int t = 0; t < threads; ++t)
        th.emplace_back([=, &sums] {
            const unsigned long long lo = n * t / threads, hi = n * (t + 1) / threads;
            z_stream z;
            memset(&z, 0, sizeof(z));
            deflateInit2(&z, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
            std::vector<unsigned char> out;
            for (unsigned long long i = lo; i < hi; ++i) {
                deflateReset(&z);
                out.resize(deflateBound(&z, (uLong)len[i]) + 16);
                z.next_in = const_cast<unsigned char*>(src + off[i]);
                z.avail_in = (unsigned)len[i];
                z.next_out = out.data();
                z.avail_out = (unsigned)out.size();
                deflate(&z, Z_SYNC_FLUSH);
                sums[t] += out.size() - z.avail_out - 4;
            }
            deflateEnd(&z);
        });
    for (auto& x : th) x.join();
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *total = 0;
    for (auto v : sums) *total += v;
    return s;
}
"""


def build_helper(tmp):
    src, so = os.path.join(tmp, "deflate_cmp.cpp"), os.path.join(tmp, "libdeflate_cmp.so")
    open(src, "w").write(HELPER)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-lz", "-o", so], check=True)
    lib = C.CDLL(so)
    lib.run.restype = C.c_double
    lib.run.argtypes = [C.c_void_p] * 3 + [C.c_ulonglong, C.c_int, C.c_void_p]
    return lib


def zsize(data, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, strategy)
    return len(c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH)) - 4


def workload(name, rng):
    """(pool of message bodies, connections, messages per connection)"""
    if name == "a":
        return [json_like(rng, 1024) for _ in range(512)], 256 * 1024, 1
    if name == "b":
        return [json_like(rng, 16384) for _ in range(64)], 64 * 1024, 4
    if name == "c":
        return [rng.integers(0, 256, 16384, dtype=np.uint8).tobytes() for _ in range(64)], 64 * 1024, 4
    return [long_text(rng, 16 << 20)], 64, 1


def run(name, dev, helper, bench):
    rng = np.random.default_rng(ord(name))
    pool, nconn, mm = workload(name, rng)
    npool, nmsg_all = len(pool), nconn * mm
    idx = np.arange(nmsg_all) % npool
    plen = np.array([len(b) for b in pool], np.uint64)
    poolsrc = np.frombuffer(b"".join(pool), np.uint8)
    poff = np.concatenate([[0], np.cumsum(plen)]).astype(np.uint64)
    reps = (nmsg_all + npool - 1) // npool
    src = torch.from_numpy(poolsrc.copy()).to(dev).repeat(reps)     # every message has its own copy of its body
    off = (np.arange(nmsg_all, dtype=np.uint64) // np.uint64(npool)) * np.uint64(len(poolsrc)) + poff[idx]
    msg = np.zeros(nmsg_all, W.DEFLATE_MSG_DTYPE)
    msg["src_off"], msg["len"], msg["type"] = off, plen[idx], 1
    caps = plen[idx]
    room_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.uint64)
    inp = int(caps.sum())
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    d_msg, d_nmsg = T(msg), torch.full((nconn,), mm, dtype=torch.int32, device=dev)
    d_off, d_cap = T(room_off[:-1]).view(torch.int64), T(caps).view(torch.int64)
    dst = torch.zeros(inp + 64, dtype=torch.uint8, device=dev)
    mres = torch.zeros(24 * nmsg_all, dtype=torch.uint8, device=dev)

    def call():
        W.batch_deflate_device(src, d_msg, d_nmsg, mm, dst, d_off, d_cap, mres)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    first = timed(call)
    r = mres.cpu().numpy().view(W.DEFLATE_MSGRES_DTYPE)
    assert (r["status"] <= W.DEFLATE_PLAIN).all(), "the device call failed on workload " + name
    out = int(r["out_len"].sum())
    for k in sorted({0, nmsg_all // 3, nmsg_all - 1}):
        room = dst[int(room_off[k]):int(room_off[k]) + int(r[k]["out_len"])].cpu().numpy().tobytes()
        back = zlib.decompressobj(-15).decompress(room + b"\x00\x00\xff\xff") if int(r[k]["status"]) == W.DEFLATE_DEFLATED else room
        assert back == pool[int(idx[k])], "wrong room on workload " + name
    warm, iters = (5, 20) if first < 1500 else (1, 5)
    for _ in range(warm - 1):
        call()
    ts = sorted(timed(call) for _ in range(iters))
    ms = ts[len(ts) // 2]
    mult = np.bincount(idx, minlength=npool)
    z1 = int(sum(int(m) * zsize(b) for m, b in zip(mult, pool)))
    zf = int(sum(int(m) * zsize(b, zlib.Z_FIXED) for m, b in zip(mult, pool)))
    # the copy that moves as many bytes: (input + output) / 2 read and as many written
    ncopy = min((inp + out) // 2 // 16 * 16, dst.numel() // 16 * 16)
    scratch = torch.empty(ncopy, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def copy():
        assert bench.websocketframeGpuCalibrate(dst.data_ptr(), scratch.data_ptr(), ncopy, 1, 1, 0, st) == 0
    for _ in range(5):
        copy()
    cs = sorted(timed(copy) for _ in range(20))
    copy_ms = cs[10] * ((inp + out) / 2 / ncopy)
    del scratch
    # the host: a share of the messages (at most 256 MiB of input), zlib level 1 on 16 threads, best of 3
    share = nmsg_all
    while share > 16 and int(room_off[share]) > (256 << 20):
        share //= 2
    hsrc = np.tile(poolsrc, (share + npool - 1) // npool)
    a_off, a_len = off[:share].copy(), plen[idx][:share].copy()
    best = None
    for _ in range(3):
        tot = C.c_ulonglong(0)
        s = helper.run(hsrc.ctypes.data, a_off.ctypes.data, a_len.ctypes.data, share, 16, C.byref(tot))
        best = s if best is None else min(best, s)
    zl = int(room_off[share]) / best / 2**30
    gibs = inp / (ms / 1e3) / 2**30
    return {"workload": name, "connections": nconn, "messages_per_connection": mm, "input_bytes": inp, "output_bytes": out,
            "deflated_messages": int((r["status"] == W.DEFLATE_DEFLATED).sum()), "plain_messages": int((r["status"] == W.DEFLATE_PLAIN).sum()),
            "zlib_level1_bytes": z1, "zlib_level1_fixed_bytes": zf, "first_call_ms": round(first, 3), "timed_calls": iters,
            "warm_calls": warm, "median_ms": round(ms, 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4),
            "input_GiBps": round(gibs, 3), "copy_same_bytes_ms": round(copy_ms, 4), "ratio_to_copy": round(copy_ms / ms, 4),
            "host_share_messages": share, "host_threads": 16, "zlib_level1_GiBps": round(zl, 3),
            "ratio_to_zlib_level1_16_threads": round(gibs / zl, 3)}


def text_sizes():
    """the host entry point on tests/inflate_cases.text(seed 1): the sizes the honesty floor is about"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import inflate_cases as IC
    rows = []
    for n in (1024, 4096, 16384):
        data = IC.text(np.random.default_rng(1), n)
        _, mr, _ = W.deflate_host(np.frombuffer(data, np.uint8), np.array([(0, n, 1, 0)], W.DEFLATE_MSG_DTYPE), [0], [n], n)
        rows.append({"len": n, "out_len": int(mr[0]["out_len"]), "status": int(mr[0]["status"]), "zlib_level1_bytes": zsize(data),
                     "zlib_level1_fixed_bytes": zsize(data, zlib.Z_FIXED)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "deflate.json"))
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
    doc = {"tool": "tools/exp_deflate.py", "device": torch.cuda.get_device_name(0),
           "method": "median of the timed calls after the warm calls, HIP events around each call; host: zlib level 1, 16 threads, "
                     "best of 3, a share of the messages, compared by input GiB/s",
           "workloads": {"a": "256 Ki connections x one 1 KiB JSON-like message",
                         "b": "64 Ki connections x 4 messages of 16 KiB, JSON-like",
                         "c": "as b, random bytes (every message PLAIN)", "d": "64 connections x one 16 MiB message (one wave each)"},
           "rows": rows, "text_seed1_sizes": text_sizes()}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
