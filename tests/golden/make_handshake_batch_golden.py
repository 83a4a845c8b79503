"""Generate tests/golden/handshake_batch.json from the REFERENCE build (run in the dev container only).

    make -C oracle ref && python tests/golden/make_handshake_batch_golden.py

Runs the reference's own websocketframeDecodeHandshakeRequest, websocketframeComputeSecAccept and
websocketframeEncodeHandshakeResponse[WithProtocol] (oracle/_ref/libwsref.so) over the directed
table of tests/handshake_cases.py and records, per case, the request and what they returned. Only
data is committed (hex inputs and outputs); no reference source.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import handshake_cases as HC  # noqa: E402


def main():
    lib = HC.reference_lib()
    assert lib is not None, "oracle/_ref/libwsref.so is not built: make -C oracle ref"
    cases = []
    for name, data in HC.directed_table():
        x = HC.expected(lib, data)
        cases.append({"name": name, "input": data.hex(), "ret": x["ret"], "key_off": x["key_off"], "key_len": x["key_len"],
                      "proto_off": None if x["proto_off"] == HC.NONE else x["proto_off"], "proto_len": x["proto_len"],
                      "accept": x["accept"].decode("ascii"), "resp": x["resp"].hex(), "resp_echo": x["resp_echo"].hex()})
    with open(os.path.join(HERE, "handshake_batch.json"), "w") as f:
        json.dump({"cases": cases}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("handshake_batch.json: %d cases" % len(cases))


if __name__ == "__main__":
    main()
