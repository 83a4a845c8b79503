"""Generate tests/golden/reassemble_ctl.json from the REFERENCE's own rx stack (dev container only).

    make -C oracle ref && python tests/golden/make_reasm_ctl_golden.py

As make_reasm_golden.py, with the on_decode glue a user of the reference writes to be RFC 6455
5.4-correct: tests/c/ctl_glue.c (built here into oracle/_ref/libctl_glue.so against the
reference's websocketframeDecode) leaves pktype = 0 for control frames, so the stream hook
delivers them straight to on_recv, past the fragment cache. Every stream of
tests/reasm_ctl_cases.py runs at several write sizes and all must agree; at least one stream's
deliveries must differ from the default glue's, else the fixture would pin nothing new.

Only data is committed (stream hashes, lengths, digests); no reference source or binary.
"""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import reasm_ctl_cases as R  # noqa: E402
import ref_reactor as X  # noqa: E402

GLUE_SO = os.path.join(X.REF_DIR, "libctl_glue.so")


def build_glue():
    """tests/c/ctl_glue.c -> oracle/_ref/libctl_glue.so (linked against the reference codec)"""
    subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-fPIC", "-shared", "-Wall",
                    os.path.join(TESTS, "c", "ctl_glue.c"), "-I", os.path.join(X.REPO, "include"),
                    "-L", X.REF_DIR, "-lwsref", "-Wl,-rpath,$ORIGIN", "-o", GLUE_SO], check=True)
    lib = C.CDLL(GLUE_SO)
    return lib, C.cast(lib.ctl_glue_on_decode, C.c_void_p).value


def main():
    assert X.available(), "build the reference first: make -C oracle ref"
    lib, glue = build_glue()
    out = {"generator": "tests/golden/make_reasm_ctl_golden.py (reference rx stack: oracle/reactor_harness.c, "
                        "on_decode = tests/c/ctl_glue.c)",
           "glue": "on_decode = websocketframeDecode; err if ret<0, incomplete if 0, else decodelen=ret, "
                   "bodyptr=data, bodylen=(unsigned)datalen, fragment_eof=is_fin, "
                   "pktype = (type & 8) ? 0 : NETPACKET_FRAGMENT",
           "cases": []}
    differ = 0
    for name in R.CASES:
        wire, limit = R.build(name)
        runs = []
        for chunk in (7, 1500, 65536, len(wire) + 1):
            if chunk == 7 and len(wire) > 200000:
                continue
            runs.append((chunk, X.reactor_deliver(wire, chunk, limit, on_decode=glue)))
        r0 = runs[0][1]
        for chunk, r in runs[1:]:
            assert r["lens"] == r0["lens"] and (r["bodies"] == r0["bodies"]).all(), (name, chunk)
            for k in ("consumed", "frames", "detach_error", "pending", "cached"):
                assert r[k] == r0[k], (name, chunk, k)
        plain = X.reactor_deliver(wire, 1500, limit)
        if plain["lens"] != r0["lens"] or not (plain["bodies"] == r0["bodies"]).all():
            differ += 1
        out["cases"].append({
            "name": name, "wire_len": len(wire), "wire_sha256": R.sha256(wire), "readcache_max": limit,
            "write_sizes": [c for c, _ in runs],
            "msg_lens": r0["lens"], "bodies_sha256": R.sha256(r0["bodies"]),
            "consumed": r0["consumed"], "frames": r0["frames"], "detach_error": r0["detach_error"],
            "pending": r0["pending"], "cached": r0["cached"]})
        print(name, len(r0["lens"]), "messages, consumed", r0["consumed"], "of", len(wire), "detach",
              r0["detach_error"], "pending", r0["pending"], r0["cached"])
    assert differ, "no stream is delivered differently than under the default glue: the fixture pins nothing"
    print(differ, "of", len(R.CASES), "streams differ from the default glue's deliveries")
    with open(os.path.join(HERE, "reassemble_ctl.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
