"""Upgrade requests for the batch handshake's tests (include/wsframe_amd_handshake.h): the directed
table (every quirk of the reference's parse by name, SHA-1's block-count steps), the geometry
builders of the GPU suite, the seeded random requests, and `expected`, which asks a library's four
reference symbols (libwsframe_amd.so, pinned to the reference by tests/golden/handshake.json, or
the reference's own build) what a request's descriptor, accept and responses are."""
import ctypes as C
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_LIB = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libwsref.so")
KEYPAT, PROTOPAT, TERM = b"Sec-WebSocket-Key:", b"Sec-WebSocket-Protocol:", b"\r\n\r\n"
KEY = b"dGhlIHNhbXBsZSBub25jZQ=="
NONE = 0xFFFFFFFF
PAD = 32
ECHO = 1
KEY_STEPS = (19, 20, 27, 28, 83, 84, 91, 92)      # 1 + (key_len + 44) // 64 steps at 20, 84 (and 28, 92 end a pad byte's room)
FILL = b"abcdefghijklmnopqrstuvwxyz0123456789"


def filler(n, salt=0):
    """n bytes of header-like text with no NUL, no CR/LF and no 'S' (so no pattern can start in it)"""
    return bytes(FILL[(i * 7 + salt) % len(FILL)] for i in range(n))


def request(key=KEY, proto=None, line=b"GET /chat HTTP/1.1", before=b"Host: a\r\n", after=b"", key_sep=b" ",
            proto_sep=b" ", proto_first=False, tail=b""):
    k = KEYPAT + key_sep + key + b"\r\n"
    p = PROTOPAT + proto_sep + proto + b"\r\n" if proto is not None else b""
    return line + b"\r\n" + before + (p + k if proto_first else k + p) + after + b"\r\n" + tail


def directed_table():
    """(name, request bytes) rows"""
    t = [
        ("plain", request()),
        ("with protocol", request(proto=b"chat")),
        ("protocol before key", request(proto=b"chat, superchat", proto_first=True)),
        ("two keys, the first wins", request(after=KEYPAT + b" c2Vjb25k\r\n")),
        ("two protocols, the first wins", request(proto=b"one", after=PROTOPAT + b" two\r\n")),
        ("frames follow", request(proto=b"v1", tail=bytes([0x81, 0x85, 1, 2, 3, 4, 5, 6, 7, 8, 9]))),
        ("empty", b""),
        ("one byte", b"G"),
        ("terminator alone", TERM),
        ("terminator cut by 1", request()[:-1]),
        ("terminator cut by 2", request()[:-2]),
        ("terminator cut by 3", request()[:-3]),
        ("no terminator", request()[:-4] + b"\r\nX-More: 1\r\n"),
        ("NUL before the terminator", request(before=b"Host: a\0b\r\n")),
        ("NUL as first byte", b"\0" + request()),
        ("NUL inside the terminator", request()[:-2] + b"\0\n"),
        ("NUL inside the terminator, a second terminator after it", request()[:-2] + b"\0\n" + b"\r\n\r\n"),
        ("NUL right after the terminator", request(tail=b"\0\0\0")),
        ("NUL later in the frames", request(tail=bytes([0x82, 0x80, 0, 0, 0, 0]))),
        ("key only after the terminator", b"GET / HTTP/1.1\r\nHost: a\r\n\r\n" + KEYPAT + b" " + KEY + b"\r\n\r\n"),
        ("no key at all", b"GET / HTTP/1.1\r\nHost: a\r\n\r\n"),
        ("key in the request line", b"GET /?" + KEYPAT + KEY + b" HTTP/1.1\r\nHost: a\r\n\r\n"),
        ("lowercase header name", request().replace(b"Sec-WebSocket-Key", b"sec-websocket-key")),
        ("mixed case header name", request().replace(b"Sec-WebSocket-Key", b"Sec-Websocket-Key")),
        ("key pattern cut by the terminator", b"GET / HTTP/1.1\r\nSec-WebSocket-Key\r\n\r\n:" + KEY + b"\r\n\r\n"),
        ("key pattern ends at e", b"GET / HTTP/1.1\r\n" + KEYPAT + b"\r\n\r\n"),
        ("no space after the colon", request(key_sep=b"")),
        ("tabs and spaces", request(key_sep=b" \t \t", proto=b"p", proto_sep=b"\t")),
        ("skip over CRLF into the next line", request(key_sep=b" \r\n", after=b"X: y\r\n")),
        ("skip over an empty value into the next header", b"GET / HTTP/1.1\r\n" + KEYPAT + b"\r\nHost: a\r\n\r\n"),
        ("skip over bytes >= 0x80", request(key_sep=b" \x80\xff\xc3\xa9 ")),
        ("key skip reaches e", b"GET / HTTP/1.1\r\nHost: a\r\n" + KEYPAT + b"  \r\n\r\n"),
        ("key skip of 0x80 bytes reaches e", b"GET / HTTP/1.1\r\n" + KEYPAT + b"\x80\x90\r\n\r\n"),
        ("protocol skip reaches e", b"GET / HTTP/1.1\r\n" + KEYPAT + b" " + KEY + b"\r\n" + PROTOPAT + b" \r\n\r\n"),
        ("protocol skip crosses a line", request(proto=b"", proto_sep=b" ", after=b"Origin: x\r\n")),
        ("protocol pattern cut by the terminator", request()[:-2] + PROTOPAT[:20] + b"\r\n\r\n"),
        ("protocol with bytes >= 0x80", request(proto=b"caf\xc3\xa9")),
        ("key ends at e", b"GET / HTTP/1.1\r\n" + KEYPAT + b" " + KEY + b"\r\n\r\n"),
        ("key of one byte", request(key=b"x")),
        ("key with inner spaces", request(key=b"a b  c")),
        ("value holds a lone LF", request(key=b"ab\ncd")),
        ("long protocol", request(proto=filler(300, 3))),
        ("long request", request(before=b"Cookie: " + filler(2500, 1) + b"\r\n", proto=b"chat")),
        ("bare terminator first", TERM + request()),
    ]
    for n in KEY_STEPS + (55, 56, 119, 120, 160):
        t.append(("key of %d bytes" % n, request(key=filler(n, n))))
    names = [n for n, _ in t]
    assert len(set(names)) == len(names)
    return t


# ------------------------------------------------------------------ expected values from a library

def load_reference_symbols(path):
    lib = C.CDLL(path)
    vp, u32 = C.c_void_p, C.c_uint
    lib.websocketframeComputeSecAccept.restype = vp
    lib.websocketframeComputeSecAccept.argtypes = [vp, u32, vp]
    lib.websocketframeDecodeHandshakeRequest.restype = C.c_int
    lib.websocketframeDecodeHandshakeRequest.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u32), C.POINTER(vp),
                                                         C.POINTER(u32)]
    lib.websocketframeEncodeHandshakeResponse.restype = vp
    lib.websocketframeEncodeHandshakeResponse.argtypes = [vp, u32, vp]
    lib.websocketframeEncodeHandshakeResponseWithProtocol.restype = vp
    lib.websocketframeEncodeHandshakeResponseWithProtocol.argtypes = [vp, u32, vp, u32]
    lib.websocketframeFreeString.restype = None
    lib.websocketframeFreeString.argtypes = [vp]
    return lib


def host_symbols():
    """the four reference symbols of libwsframe_amd.so (a handle of its own: the argument types
    above, not util_amd's)"""
    from util_amd import _lib
    _lib.load_lib()
    return load_reference_symbols(_lib.LIB_PATH)


def reference_lib():
    """the reference's own build where it is present, else None"""
    return load_reference_symbols(REF_LIB) if os.path.exists(REF_LIB) else None


def expected(lib, data):
    """{ret, key_off, key_len, proto_off, proto_len, accept, resp, resp_echo} of one request, from
    the four reference symbols of `lib`; offsets at their rest values unless ret > 0"""
    buf = C.create_string_buffer(bytes(data) + b"\xEE" * PAD, len(data) + PAD)
    base = C.addressof(buf)
    sk, skl, sp, spl = C.c_void_p(0), C.c_uint(0), C.c_void_p(0), C.c_uint(0)
    ret = lib.websocketframeDecodeHandshakeRequest(base, len(data), C.byref(sk), C.byref(skl), C.byref(sp), C.byref(spl))
    out = {"ret": ret, "key_off": 0, "key_len": 0, "proto_off": NONE, "proto_len": 0, "accept": b"", "resp": b"",
           "resp_echo": b""}
    if ret <= 0:
        return out
    out["key_off"], out["key_len"] = sk.value - base, skl.value
    if sp.value:
        out["proto_off"], out["proto_len"] = sp.value - base, spl.value
    acc = C.create_string_buffer(60)
    assert lib.websocketframeComputeSecAccept(sk.value, skl.value, acc)
    out["accept"] = acc.value
    assert len(acc.value) == 28
    rb = C.create_string_buffer(162)
    lib.websocketframeEncodeHandshakeResponse(acc, 28, rb)
    out["resp"] = rb.value
    p = lib.websocketframeEncodeHandshakeResponseWithProtocol(acc, 28, sp.value, spl.value)
    assert p
    out["resp_echo"] = C.string_at(p)
    lib.websocketframeFreeString(p)
    return out


def expected_record(exp, flags, has_resp, resp_cap):
    """the descriptor fields the interface derives from an `expected` dict"""
    resp = exp["resp_echo"] if flags & ECHO else exp["resp"]
    fl = 0
    if exp["ret"] > 0 and has_resp:
        fl = 2 if len(resp) > resp_cap else 1
    return (exp["ret"], exp["key_off"], exp["key_len"], exp["proto_off"], exp["proto_len"], len(resp), fl, 0)


# ------------------------------------------------------------------ geometry builders (GPU suite)

def terminator_at(off):
    """a complete request whose terminator starts at `off` (off >= 0): key and protocol as early as
    they fit, filler up to the terminator"""
    head = KEYPAT + b" " + KEY + b"\r\n" + PROTOPAT + b" chat\r\nX: "
    body = (head + filler(off, off))[:off] if off >= len(head) else filler(off, off)
    return body + TERM + b"\x81\x00"


def pattern_at(off, which):
    """a complete request whose key (which 0) or protocol (which 1) pattern starts at `off`, the
    other header after it"""
    k, p = KEYPAT + b" " + KEY + b"\r\n", PROTOPAT + b" chat\r\n"
    lead = (b"G" + filler(off, off))[:off] if off else b""
    return lead + (k + p if which == 0 else p + k) + b"\r\n"


def value_ending_at(edge, n, which):
    """a complete request whose key (which 0) or protocol (which 1) value of n bytes ends (its
    '\\r') at offset `edge`"""
    pat = (KEYPAT, PROTOPAT)[which] + b" "
    other = (PROTOPAT + b" chat\r\n", KEYPAT + b" " + KEY + b"\r\n")[which]
    lead = edge - n - len(pat)
    assert lead >= len(other)
    return other + filler(lead - len(other) - 2, n) + b"\r\n" + pat + filler(n, n + 1) + b"\r\n\r\n"


# ------------------------------------------------------------------ seeded random requests

SEPS = [b" ", b" ", b" ", b"", b"\t", b"  ", b" \r\n", b"\r\n ", b" \x80\xfe ", b"\r\n\t"]


def random_request(rng):
    """one request of 20..3000 bytes; every class of result has a share of the draws"""
    size = rng.choice((rng.randint(20, 200), rng.randint(200, 900), rng.randint(900, 3000)))
    klen = rng.choice((24, 24, 24, rng.randint(1, 160)))
    key = filler(klen, rng.randrange(36))
    proto = rng.choice((None, None, b"chat", filler(rng.randint(1, 40), 5)))
    ks, ps = rng.choice(SEPS), rng.choice(SEPS)
    after = b"X-After: 1\r\n" if b"\n" in ks or b"\n" in ps or rng.random() < 0.3 else b""
    cls, pf = rng.random(), rng.random() < 0.3
    room = size - len(request(key=key, proto=proto, key_sep=ks, proto_sep=ps, proto_first=pf, before=b"", after=after))
    before = b""
    if room > 12:
        before = b"Cookie: " + filler(room - 10, rng.randrange(36)) + b"\r\n"
    req = request(key=key, proto=proto, key_sep=ks, proto_sep=ps, proto_first=pf, before=before, after=after)
    tail = bytes(rng.randrange(256) for _ in range(rng.choice((0, 0, 2, 9, 40))))
    if cls < 0.55:
        out = req + tail
    elif cls < 0.62:
        out = req[:len(req) - rng.randint(1, 4)]                       # the terminator is cut
    elif cls < 0.70:
        pos = rng.randrange(len(req) - 3)
        out = req[:pos] + b"\0" + req[pos + 1:] + tail                 # a NUL before the terminator's end
    elif cls < 0.76:
        out = req.replace(b"Sec-WebSocket-Key", b"sec-websocket-key") + tail
    elif cls < 0.82:
        out = request(line=b"GET / HTTP/1.1", before=before, key=b"", key_sep=rng.choice((b"", b" ", b" \x80")),
                      after=b"") + tail                                 # the key's skip reaches e
    elif cls < 0.88:
        cut = req.index(KEYPAT)
        out = req[:cut] + b"\r\n\r\n" + req[cut:] + tail if cut >= 2 else req + tail   # the key only after the terminator
    else:
        out = req + b"\0" + tail                                       # a NUL after the terminator
    out = out[:3000]
    return out if len(out) >= 20 else out + b"#" * (20 - len(out))


def random_requests(n=4096, seed=6455):
    rng = random.Random(seed)
    return [random_request(rng) for _ in range(n)]


def skip_crosses_line(data, exp):
    """a counted header's value skip passed a line end"""
    if exp["ret"] <= 0:
        return False
    e = exp["ret"] - 4
    k = data.find(KEYPAT)
    hit = b"\n" in data[k + len(KEYPAT):exp["key_off"]]
    p = data.find(PROTOPAT)
    if exp["proto_off"] != NONE and 0 <= p and p + len(PROTOPAT) <= e:
        hit = hit or b"\n" in data[p + len(PROTOPAT):exp["proto_off"]]
    return hit


def coverage(reqs, exps):
    """the share of the requests in each class the suite must see"""
    n = float(len(reqs))
    c = {"ret > 0": 0, "ret == 0": 0, "ret == -1": 0, "protocol present": 0, "protocol absent": 0, "skip crosses a line": 0}
    for d, x in zip(reqs, exps):
        c["ret > 0"] += x["ret"] > 0
        c["ret == 0"] += x["ret"] == 0
        c["ret == -1"] += x["ret"] == -1
        c["protocol present"] += x["ret"] > 0 and x["proto_off"] != NONE
        c["protocol absent"] += x["ret"] > 0 and x["proto_off"] == NONE
        c["skip crosses a line"] += skip_crosses_line(d, x)
    return {k: v / n for k, v in c.items()}


def pack(reqs, bases=None, gap_byte=0xEE, align=1):
    """requests laid into one batch: (numpy uint8 buffer with PAD bytes after the last segment,
    seg_off, seg_len). bases: explicit segment offsets (ascending, non-overlapping); else each
    segment starts at the next multiple of `align` after the previous one's end."""
    off, pos = [], 0
    for i, r in enumerate(reqs):
        if bases is not None:
            pos = bases[i]
        else:
            pos = (pos + align - 1) // align * align
        off.append(pos)
        pos += len(r)
    buf = np.full(pos + PAD, gap_byte, np.uint8)
    for o, r in zip(off, reqs):
        buf[o:o + len(r)] = np.frombuffer(r, np.uint8)
    return buf, np.array(off, np.uint64), np.array([len(r) for r in reqs], np.uint64)
