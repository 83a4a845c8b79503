"""Child process of tests/test_gpu_host_edges.py::test_mixed_paths_in_one_call: a fresh process, so the
host pipeline's slots are in a known state. argv: "unprimed" | "primed", then the mixed layout's name.
Runs the mixed call through batch_decode_host and batch_decode_host_multi on [0, 0] under "path" -1
and prints one JSON line: per entry point the return (0, or the error text) and whether the host
image, the results and the descriptors equal the oracle's."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import host_cases as H  # noqa: E402
from oracle_lib import oracle_segments, used_descs  # noqa: E402
from util_amd import wsframe as W  # noqa: E402


def run(layout, call):
    image = H.filled(layout)
    so, sl, mf = layout.so, layout.sl, layout.max_frames
    want = image.copy()
    od, orr = oracle_segments(want, so, sl, mf)
    hb = image.copy()
    try:
        gd, gr = call(hb, np.asarray(so, np.uint64), np.asarray(sl, np.uint64), mf)
    except RuntimeError as e:
        return {"rc": str(e), "image": bool(np.array_equal(hb, want)), "res": False, "desc": False}
    unused_zero = all(not gd[s * mf + int(gr[s]["n_frames"]):(s + 1) * mf].view(np.uint8).any() for s in range(len(so)))
    return {"rc": 0, "image": bool(np.array_equal(hb, want)), "res": bool(np.array_equal(gr, orr)),
            "desc": bool(np.array_equal(used_descs(gd, gr, mf), used_descs(od, orr, mf))) and unused_zero}


def main():
    primed, name = sys.argv[1] == "primed", sys.argv[2]
    mixed = {L.name: L for L in H.mixed_layouts()}[name]
    W.set_option("host_chunk_mb", 1)
    W.set_option("path", -1)
    out = {"primed": primed, "layout": name}
    if primed:
        out["prime"] = run(H.prime_layout(), W.batch_decode_host)
    out["host"] = run(mixed, W.batch_decode_host)
    out["multi"] = run(mixed, lambda b, o, l, mf: W.batch_decode_host_multi(b, o, l, mf, [0, 0]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
