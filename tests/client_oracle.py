"""The client handshake's model (include/wsframe_amd_client.h), written from the header's wording
with bytes.split, .lower(), hashlib and base64. It shares no code with util_amd/csrc/ws_client.h:
every expectation of tests/test_client_host.py and tests/test_gpu_client.py comes from here (or
from the reference-pinned host symbols), never from the code under test."""
import base64
import hashlib

NONE = 0xFFFFFFFF
PAD = 32
GUID = b"258EAFA5-E914-47DA-95CA-C5AB0DC85B11"
REQ_WRITTEN, REQ_NO_SPACE, ERR_RANGE, ERR_BYTES, ERR_SEG_LEN = 1, 2, 4, 8, 16
OK, STATUS, UPGRADE, CONNECTION, ACCEPT, EXTENSION, PROTOCOL, TOO_LONG = range(8)
REASON_NAMES = ("ok", "STATUS", "UPGRADE", "CONNECTION", "ACCEPT", "EXTENSION", "PROTOCOL", "TOO_LONG")
WS = b" \t"


def key_of(nonce):
    assert len(nonce) == 16
    return base64.b64encode(nonce)


def expect_of(nonce):
    """the 32 bytes of d_expect: 28 accept characters and 4 zero bytes"""
    return base64.b64encode(hashlib.sha1(key_of(nonce) + GUID).digest()) + b"\0\0\0\0"


def request(path, nonce, proto=b"", host=b"", templates=None):
    """the request's bytes; templates: the two format strings parsed out of wsframe_amd.h (else the
    text is written out here)"""
    key = key_of(nonce)
    if templates is not None:
        plain, with_proto = templates
        text = with_proto % (path, key, proto) if proto else plain % (path, key)
    else:
        text = (b"GET " + path + b" HTTP/1.1\r\nUpgrade: websocket\r\nConnection: Upgrade\r\nSec-WebSocket-Version: 13\r\n"
                b"Sec-WebSocket-Key: " + key + b"\r\n" + (b"Sec-WebSocket-Protocol: " + proto + b"\r\n" if proto else b"") +
                b"\r\n")
    if host:
        line, rest = text.split(b"\r\n", 1)
        text = line + b"\r\nHost: " + host + b"\r\n" + rest
    return text


def request_record(path, nonce, proto=b"", host=b"", req_cap=None, in_range=True):
    """(req_len, key_off, flags, reserved), the request bytes or None, the expect bytes or None"""
    err = 0
    if not in_range or len(path) == 0:
        err |= ERR_RANGE
    if in_range and (any(b <= 0x20 or b == 0x7F for b in path) or any(b < 0x20 or b == 0x7F for b in proto + host)):
        err |= ERR_BYTES
    if err:
        return (0, 0, err, 0), None, None
    text = request(path, nonce, proto, host)
    key_off = text.index(b"Sec-WebSocket-Key: ") + 19
    if req_cap is None:
        return (len(text), key_off, 0, 0), None, expect_of(nonce)
    if len(text) > req_cap:
        return (len(text), key_off, REQ_NO_SPACE, 0), None, expect_of(nonce)
    return (len(text), key_off, REQ_WRITTEN, 0), text, expect_of(nonce)


def fold(b):
    return b.lower()                       # bytes.lower folds A-Z only


def elements(value):
    return [x.strip(WS) for x in value.split(b",")]


def verify(data, expect, offered=b"", max_head=0):
    """(ret, reason, status, proto_off, proto_len, accept_off, flags, reserved) of one segment"""
    if len(data) >= 1 << 31:
        return (-1, 0, 0, NONE, 0, NONE, ERR_SEG_LEN, 0)
    head = data[:max_head] if max_head else data
    e = head.find(b"\r\n\r\n")
    if e < 0:
        if max_head and len(data) >= max_head:
            return (-1, TOO_LONG, 0, NONE, 0, NONE, 0, 0)
        return (0, 0, 0, NONE, 0, NONE, 0, 0)
    lines, pos, offs = data[:e].split(b"\r\n"), 0, []
    for ln in lines:
        offs.append(pos)
        pos += len(ln) + 2
    headers = []                           # (folded name, value, value offset)
    for ln, off in zip(lines[1:], offs[1:]):
        if ln[:1] in (b" ", b"\t") or b":" not in ln:
            continue
        name, raw = ln.split(b":", 1)
        if not name:
            continue
        value = raw.strip(WS)
        voff = off + len(name) + 1 + (len(raw) - len(raw.lstrip(WS))) if value else off + len(ln)
        headers.append((fold(name), value, voff))

    def named(n):
        return [(v, o) for k, v, o in headers if k == n]

    sl = lines[0]
    status = 0
    if (len(sl) >= 12 and sl[:7] == b"HTTP/1." and sl[7:8].isdigit() and sl[8:9] == b" " and sl[9:12].isdigit()):
        status = int(sl[9:12])
    acc = named(b"sec-websocket-accept")
    accept_off = acc[0][1] if acc else NONE
    protos = named(b"sec-websocket-protocol")
    up = named(b"upgrade")
    reason = OK
    if not (sl[:12] == b"HTTP/1.1 101" and (len(sl) == 12 or sl[12:13] == b" ")):
        reason = STATUS
    elif not (up and fold(up[0][0]) == b"websocket"):
        reason = UPGRADE
    elif not any(fold(x) == b"upgrade" for v, _o in named(b"connection") for x in elements(v)):
        reason = CONNECTION
    elif not (acc and acc[0][0] == expect[:28] and len(acc[0][0]) == 28):
        reason = ACCEPT
    elif any(v for v, _o in named(b"sec-websocket-extensions")):
        reason = EXTENSION
    elif protos and not (len(protos) == 1 and protos[0][0] and offered and protos[0][0] in elements(offered)):
        reason = PROTOCOL
    if reason:
        return (-1, reason, status, NONE, 0, accept_off, 0, 0)
    po, pl = (protos[0][1], len(protos[0][0])) if protos else (NONE, 0)
    return (e + 4, 0, status, po, pl, accept_off, 0, 0)


def result_class(rec):
    """the class of a verify record, for the coverage condition"""
    if rec[0] > 0:
        return "ok with protocol" if rec[3] != NONE else "ok"
    if rec[0] == 0:
        return "incomplete"
    return REASON_NAMES[rec[1]]
