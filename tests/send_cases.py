"""Cases of the batch message send (tests/test_send_host.py, tests/test_gpu_send.py): the directed
table — the smallest shapes that can go wrong — and seeded random lists. A case is a batch:
dict(name, conns = [[(src_off, len, type)]], frags = [F per connection], role = client?). All
cases read one body buffer, source(), and get their keys from keys_for()."""
import numpy as np

import send_oracle as S

SRC_LEN = 1 << 18
BIG = 140000                      # the table keeps a message at or below this


def source():
    return np.random.default_rng(20).integers(0, 256, SRC_LEN, dtype=np.uint8)


def keys_for(case, max_msgs):
    if not case["role"]:
        return None
    n = len(case["conns"]) * max_msgs
    return (np.arange(1, n + 1, dtype=np.uint64) * 0x9E3779B1 % (1 << 32)).astype(np.uint32) | np.uint32(0x01000000)


SERVER_F = [0, 1, 2, 3, 125, 126, 127, 129, 130, 65535, 65536, 65539, 65545, 65546, 0xFFFFFFFF]
CLIENT_F = [6, 7] + [f + 4 for f in SERVER_F[4:-1]] + [0xFFFFFFFF]


def lengths(F, role):
    """the message lengths the table sends on a connection with fragment size F"""
    shard = S.shard_of(F, role)
    ls = [0, 1, 125, 126, 65535, 65536]
    if shard and shard < BIG:
        ls += [shard - 1, shard, shard + 1, 2 * shard] + ([3 * shard, 7 * shard + 2] if shard < 1000 else [])
    return sorted(set(l for l in ls if 0 <= l <= BIG and (shard >= 3 or l <= 4096)))


def fragment_rows():
    """one batch per role: a connection per fragment size with every length of lengths(); for a size
    too small to carry a byte, an empty message alone (sent, as the reference does) and an empty one
    followed by a one-byte one (the connection fails at index 1)"""
    out = []
    for role, fs in ((False, SERVER_F), (True, CLIENT_F)):
        conns, frags = [], []
        for F in fs:
            if not S.shard_of(F, role):
                conns += [[(5, 0, 1)], [(5, 0, 2), (6, 1, 2), (7, 0, 1)]]
                frags += [F, F]
                continue
            pos, c = 0, []
            for n, L in enumerate(lengths(F, role)):
                if pos + L > SRC_LEN:
                    pos = n                                   # (ranges may overlap; keep the phases moving)
                c.append((pos, L, 1 + n % 2))
                pos += L + 1
            conns.append(c)
            frags.append(F)
        out.append(dict(name="fragment sizes, %s role" % ("client" if role else "server"), conns=conns, frags=frags, role=role))
    return out


def list_rows():
    K = S.SKIP
    m = lambda o, n, t=2: (o, n, t)
    out = []
    for role in (False, True):
        conns = [
            [],                                               # nmsg = 0
            [m(0, 0, K)],                                     # SKIP as the only entry
            [m(0, 0, K), m(1, 1, K), m(1 << 62, 1 << 62, K)],  # ... several, one with a range nobody checks
            [m(9, 9, K), m(0, 10), m(20, 200, 1)],            # SKIP first
            [m(0, 10), m(9, 9, K), m(20, 200, 1)],            # middle
            [m(0, 10), m(20, 200, 1), m(9, 9, K)],            # last
            [m(3, 30)],                                       # good
            [m(SRC_LEN, 1), m(0, 10)],                        # a range error in message 0, between two good ones
            [m(40, 400, 1)],                                  # good
            [m(0, 10), m(1, 0), m(SRC_LEN - 1, 2)],           # a range error in the last message
            [m(SRC_LEN, 0), m(SRC_LEN - 1, 1), m(0, SRC_LEN)],  # the range's edges: all inside
            [m((1 << 64) - 1, 2)],                            # src_off + len wraps
            [m(2, (1 << 64) - 1)],
            [m(i, 3, i) for i in range(16)],                  # opcodes 0 to 15
            [m(i, 0, i) for i in range(16)],                  # ... on empty messages
            [m(0, 5, 0x1F2)],                                 # only the low four bits are written
        ]
        out.append(dict(name="lists, %s role" % ("client" if role else "server"), conns=conns,
                        frags=[S.FRAG_DEFAULT] * len(conns), role=role))
        out.append(dict(name="lists at F = 100, %s role" % ("client" if role else "server"), conns=conns,
                        frags=[100] * len(conns), role=role))
    return out


def directed_table():
    return fragment_rows() + list_rows()


def random_cases(seed=11, n=24):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        role = bool(k & 1)
        nseg = int(rng.integers(1, 12))
        conns, frags = [], []
        for _ in range(nseg):
            F = int(rng.choice([0xFFFFFFFF, 2 + 4 * role, 3 + 4 * role, 7 + 4 * role, 20, 126, 130, 300, 4100, 65546, int(rng.integers(0, 70000))]))
            c = []
            for _ in range(int(rng.integers(0, 9))):
                kind = int(rng.integers(0, 20))
                L = int(rng.choice([0, 1, 2, 15, 16, 17, 125, 126, int(rng.integers(0, 3000)), int(rng.integers(0, 70000))]))
                if F < 16 + 4 * role:
                    L = min(L, 300)
                so = int(rng.integers(0, SRC_LEN - L + 1))
                if kind == 0:
                    c.append((so, L, S.SKIP))
                elif kind == 1:
                    c.append((SRC_LEN - L + 1, L, 2))
                else:
                    c.append((so, L, int(rng.integers(0, 16))))
            conns.append(c)
            frags.append(F)
        out.append(dict(name="random %d" % k, conns=conns, frags=frags, role=role))
    return out


def expect(case, src, max_msgs=None):
    """(d_msg records, d_nmsg, max_msgs, keys, model outputs (tx, tx_off, msg_tx_off, res))"""
    msg, nmsg, mm = S.pack(case["conns"], max_msgs)
    keys = keys_for(case, mm)
    return msg, nmsg, mm, keys, S.batch(src, case["conns"], case["frags"], keys, mm)
