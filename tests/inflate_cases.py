"""Inputs for the inflate tests (test_inflate_host.py, test_gpu_inflate.py): permessage-deflate
bodies made by zlib (raw deflate, Z_SYNC_FLUSH, the 4-byte tail stripped) and hand-built bit streams
for what zlib never emits. Expected outputs come from inflate_oracle.py, never from here."""
import zlib

import numpy as np

TAIL = b"\x00\x00\xff\xff"


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out = c.compress(bytes(data)) + c.flush(zlib.Z_SYNC_FLUSH)
    assert out.endswith(TAIL)
    return out[:-4]


class Bits:
    """a DEFLATE bit stream: fields least significant bit first, Huffman codes most significant first"""

    def __init__(self):
        self.v, self.n = 0, 0

    def bits(self, value, n):
        self.v |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        return self

    def code(self, code_len):
        code, n = code_len
        return self.bits(int(format(code, "0%db" % n)[::-1], 2), n)

    def done(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canon(lengths):
    """symbol -> (code, length) of the canonical code (RFC 1951 section 3.2.2), whatever the set's state"""
    out, code = {}, 0
    for ln in range(1, 16):
        for s, v in enumerate(lengths):
            if v == ln:
                out[s] = (code, ln)
                code += 1
        code <<= 1
    return out


ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_DEFAULT = [4] * 13 + [5] * 6          # a complete code-length code over all 19 symbols


def fixed_codes():
    return canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), canon([5] * 32)


def length_code(n):
    """a match length 3..258 -> (literal/length symbol, extra bits, their value)"""
    if n == 258:
        return 285, 0, 0
    if n < 11:
        return 254 + n, 0, 0
    e = (n - 3).bit_length() - 3
    return 257 + 4 * (e + 1) + ((n - 3) >> e & 3), e, (n - 3) & ((1 << e) - 1)


def dist_code(d):
    """a distance 1..32768 -> (distance symbol, extra bits, their value)"""
    if d < 5:
        return d - 1, 0, 0
    e = (d - 1).bit_length() - 2
    return 2 * (e + 1) + ((d - 1) >> e & 1), e, (d - 1) & ((1 << e) - 1)


def fixed_block(ops, final=1):
    """one fixed-Huffman block from literals (ints) and matches ((length, distance)), closed by 256"""
    lf, df = fixed_codes()
    w = Bits().bits(final, 1).bits(1, 2)
    for op in ops:
        if isinstance(op, int):
            w.code(lf[op])
        else:
            ls, le, lv = length_code(op[0])
            ds, de, dv = dist_code(op[1])
            w.code(lf[ls]).bits(lv, le).code(df[ds]).bits(dv, de)
    return w.code(lf[256]).done()


def fixed_block_matches(body):
    """[(output position, length, distance symbol, extra value, distance)] of a body that is one fixed
    block, read with the fixed code written out here (a light parse, as max_code_length)"""
    v, pos, out, found = int.from_bytes(body, "little"), 3, 0, []
    assert (v >> 1) & 3 == 1

    def take(n):
        nonlocal pos
        r = v >> pos & ((1 << n) - 1)
        pos += n
        return r

    def code(n):
        r = 0
        for _ in range(n):
            r = r << 1 | take(1)
        return r
    while True:
        c = code(7)
        if c <= 0b0010111:
            s = 256 + c
        else:
            c = c << 1 | take(1)
            if 0x30 <= c <= 0xBF:
                s = c - 0x30
            elif 0xC0 <= c <= 0xC7:
                s = 280 + c - 0xC0
            else:
                s = 144 + (c << 1 | take(1)) - 0x190
        if s < 256:
            out += 1
            continue
        if s == 256:
            return found
        i = s - 257
        le = 0 if i < 8 or i == 28 else (i >> 2) - 1
        n = 3 + i if i < 8 else (258 if i == 28 else 3 + ((4 + (i & 3)) << le)) + take(le)
        d = code(5)
        de = 0 if d < 4 else (d >> 1) - 1
        x = take(de)
        found.append((out, n, d, x, (1 + d if d < 4 else 1 + ((2 + (d & 1)) << de)) + x))
        out += n


def played(ops):
    """the bytes a list of literals and (length, distance) matches stands for"""
    out = bytearray()
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        else:
            for _ in range(op[0]):
                out.append(out[-op[1]])
    return bytes(out)


FAR_OPS = [120, 121, 122] + [(258, 1)] * 126 + [(257, 1), (10, 32768)] + [(258, 32768)] * 4


def far_match(short=0):
    """33 KiB whose end repeats its start at distance 32,768: three literals (two when `short`: the
    distance is then one past the output), a run at distance 1 up to 32,768 bytes, then five matches
    at distance 32,768 — distance symbol 29 with all 13 extra bits set, the copy's source the
    message's first byte"""
    return fixed_block(FAR_OPS[short:])


def dyn(litlens, distlens, seq=None, cl=None, final=1, nlen=None, ndist=None):
    """a dynamic block's header. seq: the code-length symbols [(sym, extra value)] (default: one per
    length, no repeats); cl: the 19 code-length code lengths. Returns (Bits, literal/length codes,
    distance codes)."""
    cl = CL_DEFAULT if cl is None else cl
    nlen = len(litlens) if nlen is None else nlen
    ndist = len(distlens) if ndist is None else ndist
    if seq is None:
        seq = [(v, 0) for v in list(litlens) + list(distlens)]
    w = Bits().bits(final, 1).bits(2, 2).bits(nlen - 257, 5).bits(ndist - 1, 5)
    ncode = max([4] + [k + 1 for k in range(19) if cl[ORDER[k]]])
    w.bits(ncode - 4, 4)
    for k in range(ncode):
        w.bits(cl[ORDER[k]], 3)
    cc = canon(cl)
    for s, x in seq:
        w.code(cc[s])
        if s >= 16:
            w.bits(x, {16: 2, 17: 3, 18: 7}[s])
    return w, canon(litlens), canon(distlens)


def lits(**kw):
    """literal/length code lengths from {symbol: length}, up to the highest symbol (at least 257 long)"""
    m = {int(k[1:]): v for k, v in kw.items()}
    n = max(257, max(m) + 1)
    return [m.get(s, 0) for s in range(n)]


def hand_built():
    """[(name, body, what the author meant: the output bytes, or None for an error)]; the model decides"""
    out = []
    lf, df = fixed_codes()
    # fixed block: 'a', then a match of length 3 at distance 2 — one past the output so far
    w = Bits().bits(1, 1).bits(1, 2).code(lf[97]).code(lf[257]).code(df[1])
    out.append(("distance one past the output", w.done() + b"\0", None))
    w = Bits().bits(1, 1).bits(1, 2).code(lf[257]).code(df[0])
    out.append(("distance at the very first symbol", w.done() + b"\0", None))
    w = Bits().bits(1, 1).bits(1, 2).code(lf[97]).code(lf[257]).code(df[0]).code(lf[256])
    out.append(("distance 1 after one literal", w.done(), b"aaaa"))
    # a repeat that crosses from the literal/length lengths into the distance lengths
    ll = lits(s97=2, s98=2, s99=3, s255=3, s256=3, s257=3)
    dl = [3] * 8
    seq = [(18, 97 - 11), (2, 0), (2, 0), (3, 0), (18, 138 - 11), (18, 17 - 11), (3, 0), (16, 6 - 3), (16, 4 - 3)]
    w, lc, dc = dyn(ll, dl, seq)
    w.code(lc[97]).code(lc[98]).code(lc[99]).code(lc[257]).code(dc[2]).code(lc[256])
    out.append(("repeat crosses into the distance lengths", w.done(), b"abcabc"))
    # a single-code distance set (incomplete, zlib's one exception), used and misused
    ll = lits(s97=1, s256=2, s257=2)
    w, lc, dc = dyn(ll, [1])
    w.code(lc[97]).code(lc[257]).code(dc[0]).code(lc[256])
    out.append(("single-code distance set", w.done(), b"aaaa"))
    w, lc, dc = dyn(ll, [1])
    w.code(lc[97]).code(lc[257]).bits(1, 1).bits(0, 16)
    out.append(("a code that is not in the incomplete distance set", w.done(), None))
    w, lc, dc = dyn(lits(s256=1), [1])
    w.code(lc[256])
    out.append(("single-code literal/length set", w.done(), b""))
    w, lc, dc = dyn(lits(s256=1), [1], final=0)
    w.bits(1, 1).bits(0, 16)
    out.append(("a code that is not in the incomplete literal/length set", w.done(), None))
    w, lc, dc = dyn(ll, [0])
    w.code(lc[97]).code(lc[256])
    out.append(("no distance code at all, none used", w.done(), b"a"))
    w, lc, dc = dyn(ll, [0])
    w.code(lc[97]).code(lc[257]).bits(0, 16)
    out.append(("no distance code at all, one used", w.done(), None))
    # the error classes
    out.append(("block type 3", bytes([0x07]), None))
    out.append(("stored LEN != ~NLEN", bytes.fromhex("0100000000"), None))
    out.append(("incomplete code-length set (the issue's)", bytes.fromhex("0500fbff68690000"), None))
    out.append(("HLIT 287", Bits().bits(1, 1).bits(2, 2).bits(30, 5).bits(0, 5).bits(0, 4).bits(0, 16).done(), None))
    out.append(("HDIST 31", Bits().bits(1, 1).bits(2, 2).bits(0, 5).bits(30, 5).bits(0, 4).bits(0, 16).done(), None))
    w, _, _ = dyn(ll, [1], seq=[(16, 0)] + [(0, 0)] * 8)
    out.append(("repeat with nothing to repeat", w.done() + b"\0\0", None))
    w, _, _ = dyn(ll, [1], seq=[(18, 127), (18, 127)])
    out.append(("repeat past HLIT + HDIST", w.done() + b"\0\0", None))
    w, _, _ = dyn(lits(s97=1, s98=1), [1])
    out.append(("no code for symbol 256", w.done() + b"\0\0", None))
    w, _, _ = dyn(ll, [1], cl=[1] * 19, seq=[])
    out.append(("over-subscribed code-length set", w.done() + b"\0\0", None))
    w, _, _ = dyn(ll, [1], cl=[1] + [0] * 18, seq=[])
    out.append(("incomplete code-length set", w.done() + b"\0\0", None))
    w, _, _ = dyn(ll, [1], cl=[0] * 19, seq=[])
    out.append(("empty code-length set, input ends in the lengths", w.done() + b"\0" * 8, b""))
    out.append(("empty code-length set, then no code for 256", w.done() + b"\0" * 64, None))
    w, _, _ = dyn(lits(s97=1, s98=1, s256=1), [1])
    out.append(("over-subscribed literal/length set", w.done() + b"\0\0", None))
    w, _, _ = dyn(ll, [1, 1, 1])
    out.append(("over-subscribed distance set", w.done() + b"\0\0", None))
    w, _, _ = dyn(lits(s97=2, s256=2), [1])
    out.append(("incomplete literal/length set", w.done() + b"\0\0", None))
    w, _, _ = dyn(ll, [2, 2])
    out.append(("incomplete distance set", w.done() + b"\0\0", None))
    w = Bits().bits(1, 1).bits(1, 2).code(lf[97]).code(lf[286])
    out.append(("literal/length symbol 286", w.done() + b"\0", None))
    w = Bits().bits(1, 1).bits(1, 2).code(lf[97]).code(lf[287])
    out.append(("literal/length symbol 287", w.done() + b"\0", None))
    w = Bits().bits(1, 1).bits(1, 2).code(lf[97]).code(lf[257]).code(df[30])
    out.append(("distance symbol 30", w.done() + b"\0", None))
    w = Bits().bits(1, 1).bits(1, 2).code(lf[97]).code(lf[257]).code(df[31])
    out.append(("distance symbol 31", w.done() + b"\0", None))
    out.append(("distance 32768 from the first byte", far_match(), played(FAR_OPS)))
    out.append(("distance 32768 one past the output", far_match(1), None))
    out.append(("BFINAL then junk", bytes.fromhex("f348cdc9c9070000"), b"Hello"))
    out.append(("the RFC's Hello", bytes.fromhex("f248cdc9c90700"), b"Hello"))
    return out


def skewed(n=24):
    """Fibonacci-like byte frequencies over n symbols: zlib's code for it reaches 15 bits"""
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    rng = np.random.default_rng(15)
    data = np.concatenate([np.full(c, 65 + i, np.uint8) for i, c in enumerate(f)])
    rng.shuffle(data)
    return data.tobytes()


def max_code_length(body):
    """the longest literal/length code length of a body's first dynamic block (a light header parse)"""
    v = int.from_bytes(body, "little")
    assert (v >> 1) & 3 == 2
    pos = 3
    nlen, ndist, ncode = (v >> pos & 31) + 257, (v >> pos + 5 & 31) + 1, (v >> pos + 10 & 15) + 4
    pos += 14
    cl = [0] * 19
    for k in range(ncode):
        cl[ORDER[k]] = v >> pos & 7
        pos += 3
    dec = {(c, n): s for s, (c, n) in canon(cl).items()}
    lens = []
    while len(lens) < nlen + ndist:
        code, n = 0, 0
        while (code, n) not in dec:
            code, n, pos = code << 1 | (v >> pos & 1), n + 1, pos + 1
        s = dec[(code, n)]
        if s < 16:
            lens.append(s)
        else:
            xb, base = {16: (2, 3), 17: (3, 3), 18: (7, 11)}[s]
            lens += [lens[-1] if s == 16 else 0] * (base + (v >> pos & ((1 << xb) - 1)))
            pos += xb
    return max(lens[:nlen])


def text(rng, n):
    words = [b"the", b"quick", b'"id":', b'"name":', b"{", b"}", b",", b"true", b"null", b"value", b"websocket", b" "]
    out = b""
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + (b"%d" % int(rng.integers(0, 1000)) if rng.random() < 0.2 else b"")
    return out[:n]


def directed_table():
    """[(name, body)]: the smallest inputs at which each part can go wrong"""
    rng = np.random.default_rng(7692)
    t = [("empty body", b""), ("one byte 00", b"\0")]
    for n in (0, 1, 65535, 65536):
        t.append(("stored %d" % n, deflate(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), 0)))
    for n in (1, 2, 3, 17, 64, 65, 127, 200, 300):
        t.append(("fixed %d" % n, deflate(text(rng, n), 6, zlib.Z_FIXED)))
        t.append(("dynamic %d" % n, deflate(text(rng, n), 9)))
    t.append(("run of one byte", deflate(b"z" * 700, 6)))
    t.append(("run of one byte, fixed", deflate(b"q" * 1000, 6, zlib.Z_FIXED)))
    head = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    far = head + rng.integers(0, 256, 32768 - 300, dtype=np.uint8).tobytes() + head + b"end"
    t.append(("head repeated after 32 KiB (zlib)", deflate(far, 9)))
    t.append(("15-bit codes", deflate(skewed(), 6, zlib.Z_HUFFMAN_ONLY)))
    t.append(("mixed 40 KiB", deflate(text(rng, 20000) + rng.integers(0, 256, 5000, dtype=np.uint8).tobytes() + text(rng, 15000), 6)))
    t += [(name, body) for name, body, _ in hand_built()]
    return t


def truncations():
    """every prefix of one 3 KB level-9 stream"""
    rng = np.random.default_rng(9)
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 8)
    body = b""
    for k in range(7):                                    # seven flushed parts: several dynamic headers to cut through
        part = text(rng, 400) if k % 2 == 0 else rng.integers(0, 256, 100, dtype=np.uint8).tobytes() + text(rng, 400)
        body += c.compress(part) + c.flush(zlib.Z_SYNC_FLUSH)
    body = body[:-4]
    return [body[:k] for k in range(len(body) + 1)]


def bit_flips():
    """all single-bit flips of a short dynamic stream"""
    rng = np.random.default_rng(11)
    body = deflate(text(rng, 260), 9)
    assert (body[0] >> 1) & 3 == 2
    out = []
    for k in range(8 * len(body)):
        b = bytearray(body)
        b[k >> 3] ^= 1 << (k & 7)
        out.append(bytes(b))
    return out


STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE]


def random_cases(n_base=5000, seed=1951):
    """seeded random bodies: compressible, incompressible and mixed inputs of 0-100 KiB at levels
    0/1/6/9 and four strategies, each also truncated, bit-flipped and spliced: 4 * n_base bodies"""
    rng = np.random.default_rng(seed)
    out, prev = [], b"\x01"
    for k in range(n_base):
        u = rng.random()
        n = int(rng.integers(0, 2049)) if u < 0.8 else (int(rng.integers(0, 16385)) if u < 0.95 else int(rng.integers(0, 102401)))
        kind = k % 3
        if kind == 0:
            data = text(rng, n)
        elif kind == 1:
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        else:
            data = text(rng, n // 2) + rng.integers(0, 256, n - n // 2, dtype=np.uint8).tobytes()
            if n > 600 and rng.random() < 0.5:
                data = data + data[:n // 3]
        body = deflate(data, int(rng.choice([0, 1, 6, 9])), STRATEGIES[int(rng.integers(0, 4))])
        out.append(body)
        out.append(body[:int(rng.integers(0, len(body) + 1))])
        b = bytearray(body)
        if b:
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(b))
        cut = int(rng.integers(0, len(body) + 1))
        out.append(body[:cut] + prev[int(rng.integers(0, len(prev) + 1)):])
        prev = body if body else prev
    return out
