"""Server responses and connection strings for the client handshake's tests
(include/wsframe_amd_client.h): the directed verify table (every reason, the status-line, name,
value, list and max_head edges by name), the geometry builders of the GPU suite, the seeded random
responses with their coverage, and the packing helpers. Expected values come from
tests/client_oracle.py."""
import random

import numpy as np

import client_oracle as CO

NONCE = bytes(range(16))
EXPECT = CO.expect_of(NONCE)
ACC = EXPECT[:28]
FILL = b"abdefghijklmnopqrtvwxyz0123456789"       # no 'c', 's', 'u': no candidate line can start in it
STATUS_LINE = b"HTTP/1.1 101 Switching Protocols"
UP, CONN, ACCEPT_NAME = b"Upgrade: websocket", b"Connection: Upgrade", b"Sec-WebSocket-Accept: "
NAMES = (b"Upgrade", b"Connection", b"Sec-WebSocket-Accept", b"Sec-WebSocket-Extensions", b"Sec-WebSocket-Protocol")


def filler(n, salt=0):
    return bytes(FILL[(i * 7 + salt) % len(FILL)] for i in range(n))


def resp(lines, tail=b""):
    return b"\r\n".join(lines) + b"\r\n\r\n" + tail


def good(acc=ACC, extra=(), status=STATUS_LINE, up=UP, conn=CONN, tail=b"", first=()):
    lines = [status] + list(first) + ([up] if up is not None else []) + ([conn] if conn is not None else [])
    if acc is not None:
        lines.append(ACCEPT_NAME + acc)
    return resp(lines + list(extra), tail)


def directed_table():
    """(name, response bytes, offered list, max_head) rows"""
    g = good()
    T4 = len(g)
    last = ACC[:-1] + (b"A" if ACC[-1:] != b"A" else b"B")
    off3 = b"a, bb ,ccc"
    P = b"Sec-WebSocket-Protocol: "
    t = [
        ("plain", g, b"", 0),
        ("frames follow", good(tail=bytes([0x81, 0x03, 1, 2, 3])), b"", 0),
        ("reason STATUS", good(status=b"HTTP/1.1 200 OK"), b"", 0),
        ("reason UPGRADE", good(up=b"Upgrade: h2c"), b"", 0),
        ("reason CONNECTION", good(conn=b"Connection: keep-alive"), b"", 0),
        ("reason ACCEPT", good(acc=b"x" * 28), b"", 0),
        ("reason EXTENSION", good(extra=[b"Sec-WebSocket-Extensions: permessage-deflate"]), b"", 0),
        ("reason PROTOCOL", good(extra=[P + b"chat"]), b"superchat", 0),
        ("reason TOO_LONG", g, b"", T4 - 1),
        ("status 200", good(status=b"HTTP/1.1 200 OK"), b"", 0),
        ("status 302", good(status=b"HTTP/1.1 302 Found"), b"", 0),
        ("status 401", good(status=b"HTTP/1.1 401 Unauthorized"), b"", 0),
        ("status line malformed", good(status=b"HTTP/1.1 1x1 Odd"), b"", 0),
        ("status line short", good(status=b"HTTP/1.1 10"), b"", 0),
        ("status line empty", good(status=b""), b"", 0),
        ("status line lower case", good(status=b"http/1.1 101 Switching Protocols"), b"", 0),
        ("HTTP/1.0", good(status=b"HTTP/1.0 101 Switching Protocols"), b"", 0),
        ("HTTP/2.0", good(status=b"HTTP/2.0 101 Switching Protocols"), b"", 0),
        ("101 with no reason phrase", good(status=b"HTTP/1.1 101"), b"", 0),
        ("101 and a space only", good(status=b"HTTP/1.1 101 "), b"", 0),
        ("1010", good(status=b"HTTP/1.1 1010 Long"), b"", 0),
        ("101 then a tab", good(status=b"HTTP/1.1 101\tX"), b"", 0),
        ("names in upper case", good().replace(b"Upgrade:", b"UPGRADE:").replace(b"Connection:", b"CONNECTION:")
         .replace(b"Sec-WebSocket-Accept:", b"SEC-WEBSOCKET-ACCEPT:"), b"", 0),
        ("names in lower case", good().replace(b"Upgrade:", b"upgrade:").replace(b"Connection:", b"connection:")
         .replace(b"Sec-WebSocket-Accept:", b"sec-websocket-accept:"), b"", 0),
        ("names in mixed case", good().replace(b"Upgrade:", b"uPgRaDe:").replace(b"Connection:", b"cONNECTIOn:")
         .replace(b"Sec-WebSocket-Accept:", b"sEC-wEBsOCKET-aCCEPt:"), b"", 0),
        ("values in other case", good(up=b"Upgrade: WebSocket", conn=b"Connection: UPGRADE"), b"", 0),
        ("accept in other case", good(acc=ACC.swapcase()), b"", 0),
        ("Connection: keep-alive, Upgrade", good(conn=b"Connection: keep-alive, Upgrade"), b"", 0),
        ("Connection: Upgrade,keep-alive", good(conn=b"Connection: Upgrade,keep-alive"), b"", 0),
        ("Connection with empty elements", good(conn=b"Connection: ,, ,\tupgrade\t ,"), b"", 0),
        ("Connection: Upgrades", good(conn=b"Connection: Upgrades, xUpgrade, Up grade"), b"", 0),
        ("Connection empty", good(conn=b"Connection:"), b"", 0),
        ("two Connection lines, the token in the second", good(conn=b"Connection: keep-alive", extra=[b"Connection: upgrade"]), b"", 0),
        ("no Connection line", good(conn=None), b"", 0),
        ("a long Connection list", good(conn=b"Connection: " + b", ".join(filler(9, i) for i in range(12)) + b" ,  upgrade"), b"", 0),
        ("name with a space before the colon", good(up=b"Upgrade : websocket"), b"", 0),
        ("name with a space before the colon, a good one later", good(up=b"Upgrade : h2c", extra=[b"Upgrade: websocket"]), b"", 0),
        ("continuation line", good(up=b"X-Any: 1\r\n Upgrade: websocket"), b"", 0),
        ("continuation line with a tab", good(up=b"X-Any: 1\r\n\tUpgrade: websocket"), b"", 0),
        ("a line without a colon", good(first=[b"Upgrade websocket"]), b"", 0),
        ("a line without a colon only", good(up=b"Upgrade websocket"), b"", 0),
        ("a line that is a colon only", good(first=[b": websocket"]), b"", 0),
        ("values with surrounding SP and HT", good(up=b"Upgrade:\t  websocket \t ", conn=b"Connection:upgrade\t",
                                                   acc=b" \t" + ACC + b"\t \t "), b"", 0),
        ("no space after the colons", good(up=b"Upgrade:websocket", conn=b"Connection:Upgrade").replace(ACCEPT_NAME, ACCEPT_NAME[:-1]), b"", 0),
        ("two Upgrade lines, the first governs (bad)", good(up=b"Upgrade: h2c", extra=[b"Upgrade: websocket"]), b"", 0),
        ("two Upgrade lines, the first governs (good)", good(extra=[b"Upgrade: h2c"]), b"", 0),
        ("Upgrade: websocket, h2c", good(up=b"Upgrade: websocket, h2c"), b"", 0),
        ("no Upgrade line", good(up=None), b"", 0),
        ("Upgrade in the status line only", good(status=STATUS_LINE + b" Upgrade: websocket", up=None), b"", 0),
        ("accept of 27 bytes", good(acc=ACC[:27]), b"", 0),
        ("accept of 29 bytes", good(acc=ACC + b"="), b"", 0),
        ("accept differs in its last byte", good(acc=last), b"", 0),
        ("accept differs in its first byte", good(acc=b"#" + ACC[1:]), b"", 0),
        ("accept with an inner space", good(acc=ACC[:10] + b" " + ACC[11:]), b"", 0),
        ("accept empty", good(acc=b""), b"", 0),
        ("no accept line", good(acc=None), b"", 0),
        ("duplicate Accept, the first governs (good)", good(extra=[ACCEPT_NAME + b"x" * 28]), b"", 0),
        ("duplicate Accept, the first governs (bad)", good(acc=b"x" * 28, extra=[ACCEPT_NAME + ACC]), b"", 0),
        ("empty Extensions value", good(extra=[b"Sec-WebSocket-Extensions:"]), b"", 0),
        ("blank Extensions value", good(extra=[b"Sec-WebSocket-Extensions: \t "]), b"", 0),
        ("an empty and a full Extensions line", good(extra=[b"Sec-WebSocket-Extensions:", b"sec-websocket-extensions: x"]), b"", 0),
        ("protocol first of the offered", good(extra=[P + b"a"]), off3, 0),
        ("protocol in the middle of the offered", good(extra=[P + b" bb\t"]), off3, 0),
        ("protocol last of the offered", good(extra=[P + b"ccc"]), off3, 0),
        ("protocol absent from the offered", good(extra=[P + b"b"]), off3, 0),
        ("protocol in another case", good(extra=[P + b"BB"]), off3, 0),
        ("protocol is the whole list", good(extra=[P + off3]), off3, 0),
        ("no protocol though offered", good(), off3, 0),
        ("duplicate protocol header", good(extra=[P + b"a", P + b"a"]), off3, 0),
        ("protocol header with nothing offered", good(extra=[P + b"a"]), b"", 0),
        ("empty protocol value", good(extra=[P]), off3, 0),
        ("empty protocol value, an empty element offered", good(extra=[P]), b"a,,b", 0),
        ("a long protocol", good(extra=[P + filler(150, 3)]), b"x, " + filler(150, 3) + b" , y", 0),
        ("a long protocol, last byte differs", good(extra=[P + filler(150, 3)]), b"x, " + filler(149, 3) + b"# , y", 0),
        ("max_head one below T + 4", g, b"", T4 - 1),
        ("max_head at T + 4", g, b"", T4),
        ("max_head one above T + 4", g, b"", T4 + 1),
        ("max_head above a cut response", g[:-1], b"", T4 + 8),
        ("max_head at a cut response's length", g[:-1], b"", T4 - 1),
        ("max_head below the frames", good(tail=b"\x81\x00" * 30), b"", T4),
        ("seg_len 0", b"", b"", 0),
        ("seg_len 0 with max_head", b"", b"", 16),
        ("one byte", b"H", b"", 0),
        ("a bare LF LF", g[:-4].replace(b"\r\n", b"\n") + b"\n\n", b"", 0),
        ("bare CR and LF inside values", good(first=[b"X-A: a\rb", b"X-B: a\nb"]), b"", 0),
        ("terminator alone", b"\r\n\r\n", b"", 0),
        ("terminator cut by 1", g[:-1], b"", 0),
        ("terminator cut by 3", g[:-3], b"", 0),
        ("a NUL in a value", good(first=[b"X-A: a\0b"]), b"", 0),
        ("a NUL first", b"\0" + g, b"", 0),
        ("headers only after the terminator", resp([STATUS_LINE]) + g, b"", 0),
        ("empty status line, then headers", resp([b"", UP, CONN, ACCEPT_NAME + ACC]), b"", 0),
        ("short lines", resp([STATUS_LINE, b"u:", b"c:", b"s:", b"u", b"", UP, CONN, ACCEPT_NAME + ACC]), b"", 0),
    ]
    names = [r[0] for r in t]
    assert len(set(names)) == len(names)
    return t


# ------------------------------------------------------------------ geometry builders (GPU suite)

def pad_line(n, salt=0):
    """a header line of exactly n bytes (n >= 6), its "\\r\\n" included, that matches no name"""
    assert n >= 6
    return b"X-" + filler(n - 5, salt) + b":\r\n"


def terminator_at(off):
    """a passing response whose terminator starts at `off`"""
    body = b"\r\n".join([STATUS_LINE, UP, CONN, ACCEPT_NAME + ACC])
    room = off - len(body) - 2
    assert room >= 4
    return body + b"\r\n" + pad_line(room + 2, off)[:-2] + b"\r\n\r\n" + b"\x81\x00"


def header_line(which, pad=b"", proto=b"chat"):
    value = (b"websocket", b"keep-alive, Upgrade", ACC, b"", proto)[which]
    return NAMES[which] + b":" + pad + value + pad[::-1]


def header_at(which, off, pad=b""):
    """a response in which header `which` (an index into NAMES) starts its line at `off`, with
    `pad` (SP/HT bytes) around its value; the other headers follow. Offer b"chat"."""
    assert off >= len(STATUS_LINE) + 2 + 6
    lines = [STATUS_LINE, pad_line(off - len(STATUS_LINE) - 2, off)[:-2], header_line(which, pad)]
    lines += [header_line(k) for k in range(5) if k != which]
    out = resp(lines, b"\x82\x00")
    assert out.index(NAMES[which] + b":") == off
    return out


def header_cases():
    """(response, offered) pairs: each of the five names starting its line at every offset
    1000..1050, and a value with 0..130 bytes of SP/HT around it at the round edge"""
    pads = [b"", b" ", b"\t ", b" \t" * 20, b" " * 63, b"\t" * 64, b" " * 65, b" " * 130]
    out = []
    for which in range(5):
        for off in range(1000, 1051):
            out.append((header_at(which, off, pads[off % len(pads)]), b"chat"))
    for n in range(131):
        out.append((header_at(n % 3, 1015, (b" \t" * 66)[:n]), b"chat"))
    return out


# ------------------------------------------------------------------ seeded random responses

CLASSES = ("ok", "ok with protocol", "incomplete") + CO.REASON_NAMES[1:]
OFFERED = (b"chat", b"a, bb ,ccc", b"v1.example,v2.example", b"x")


def recase(rng, b):
    mode = rng.randrange(4)
    return b if mode == 0 else (b.lower() if mode == 1 else (b.upper() if mode == 2 else
                                                           bytes(c ^ 0x20 if chr(c).isalpha() and rng.random() < 0.5 else c for c in b)))


def ws(rng):
    return rng.choice((b" ", b" ", b"", b"\t", b"  ", b" \t "))


def random_response(rng):
    """(response, offered, max_head): every class of result has a tenth of the draws"""
    cls = rng.choice(CLASSES)
    offered = rng.choice(OFFERED) if cls in ("ok with protocol", "PROTOCOL") or rng.random() < 0.3 else b""

    def hdr(n, v):
        return recase(rng, n) + b":" + ws(rng) + v + ws(rng)
    status = rng.choice((STATUS_LINE, b"HTTP/1.1 101", b"HTTP/1.1 101 OK"))
    up, conn = hdr(b"Upgrade", recase(rng, b"websocket")), hdr(b"Connection", rng.choice((b"Upgrade", b"keep-alive, upgrade", b"UPGRADE ,x")))
    acc = hdr(b"Sec-WebSocket-Accept", ACC)
    extra = []
    if cls == "STATUS":
        status = rng.choice((b"HTTP/1.1 200 OK", b"HTTP/1.1 302 Found", b"HTTP/1.0 101 X", b"HTTP/1.1 1010", b"junk", b""))
    elif cls == "UPGRADE":
        up = rng.choice((None, hdr(b"Upgrade", b"h2c"), hdr(b"Upgrade ", b"websocket"), b" " + up, hdr(b"Upgrade", b"websocket2")))
    elif cls == "CONNECTION":
        conn = rng.choice((None, hdr(b"Connection", b"keep-alive"), hdr(b"Connection", b"upgrades, close"), hdr(b"Connection", b"")))
    elif cls == "ACCEPT":
        bad = ACC[:-1] + bytes([ACC[-1] ^ 1])
        acc = rng.choice((None, hdr(b"Sec-WebSocket-Accept", bad), hdr(b"Sec-WebSocket-Accept", ACC[:27]),
                          hdr(b"Sec-WebSocket-Accept", ACC + b"="), hdr(b"Sec-WebSocket-Accept", ACC.swapcase())))
    elif cls == "EXTENSION":
        extra.append(hdr(b"Sec-WebSocket-Extensions", rng.choice((b"permessage-deflate", b"x"))))
    elif cls == "PROTOCOL":
        el = CO.elements(offered)
        extra += rng.choice(([hdr(b"Sec-WebSocket-Protocol", b"nope")], [hdr(b"Sec-WebSocket-Protocol", el[0])] * 2,
                             [hdr(b"Sec-WebSocket-Protocol", el[0].upper() + b"_")], [recase(rng, b"Sec-WebSocket-Protocol") + b":"]))
    elif cls == "ok with protocol":
        extra.append(hdr(b"Sec-WebSocket-Protocol", rng.choice(CO.elements(offered))))
    if cls not in ("EXTENSION",) and rng.random() < 0.2:
        extra.append(hdr(b"Sec-WebSocket-Extensions", b""))
    if cls not in ("PROTOCOL", "ok with protocol"):
        offered = offered if rng.random() < 0.5 else b""
    fill = [b"X-Pad-%d: " % i + filler(rng.choice((0, 5, 40, rng.randint(0, 700))), i) for i in range(rng.randrange(4))]
    if rng.random() < 0.15:
        fill.append(b"Server: " + filler(rng.randint(800, 2200), 9))
    lines = [x for x in [up, conn, acc] + extra + fill if x is not None]
    rng.shuffle(lines)
    out = resp([status] + lines)
    tail = bytes(rng.randrange(256) for _ in range(rng.choice((0, 0, 2, 9, 40))))
    max_head = 0
    if cls == "incomplete":
        out = out[:len(out) - rng.randint(1, 4)] if rng.random() < 0.7 else out[:rng.randrange(len(out) - 3)]
        if rng.random() < 0.3:
            max_head = len(out) + rng.randint(1, 64)
    elif cls == "TOO_LONG":
        max_head = rng.randint(1, len(out) - 1)
        out = out + tail if rng.random() < 0.5 else out[:rng.randint(max_head, len(out))]
    else:
        if rng.random() < 0.3:
            max_head = len(out) + rng.choice((0, 1, 100))
        out += tail
    return out, offered, max_head


def random_responses(n=4096, seed=6455):
    rng = random.Random(seed)
    return [random_response(rng) for _ in range(n)]


def coverage(cases):
    """the share of the cases in each class, on the model's own results"""
    c = dict.fromkeys(CLASSES, 0)
    for d, off, mh in cases:
        c[CO.result_class(CO.verify(d, EXPECT, off, mh))] += 1
    return {k: v / float(len(cases)) for k, v in c.items()}


# ------------------------------------------------------------------ packing

def pack(segs, bases=None, gap_byte=0xEE, align=1):
    """segments laid into one batch: (numpy uint8 buffer with PAD bytes after the last segment,
    seg_off, seg_len). bases: explicit segment offsets (ascending, non-overlapping); else each
    segment starts at the next multiple of `align` after the previous one's end."""
    off, pos = [], 0
    for i, r in enumerate(segs):
        pos = bases[i] if bases is not None else (pos + align - 1) // align * align
        off.append(pos)
        pos += len(r)
    buf = np.full(pos + CO.PAD, gap_byte, np.uint8)
    for o, r in zip(off, segs):
        buf[o:o + len(r)] = np.frombuffer(r, np.uint8)
    return buf, np.array(off, np.uint64), np.array([len(r) for r in segs], np.uint64)


def pool(strings):
    """the string pool of a list of (path, proto, host): (numpy uint8 pool, entry records as a
    structured array of the interface's layout)"""
    dt = np.dtype([("path_off", "<u8"), ("proto_off", "<u8"), ("host_off", "<u8"), ("path_len", "<u4"),
                   ("proto_len", "<u4"), ("host_len", "<u4"), ("reserved", "<u4", (3,))])
    ent = np.zeros(len(strings), dt)
    blob = bytearray()
    for i, (path, proto, host) in enumerate(strings):
        for name, b in (("path", path), ("proto", proto), ("host", host)):
            ent[i][name + "_off"], ent[i][name + "_len"] = len(blob), len(b)
            blob += b
    return np.frombuffer(bytes(blob) + b"\0", np.uint8).copy(), ent
