"""The inflate kernel's Io (util_amd/csrc/ws_inflate.hip) on the device, at the geometries
inflate_dev_cases.py builds for it: the wave-wide match copy over p x dist x len, token streams that
take and skip the `fenced` wait behind full and partial literal runs, the stored copy at every
(source, destination) residue mod 16 and into the virtual tail, the 256-byte input window at every
source alignment, a seeded sweep of zlib's bodies and their mutations, and offsets past 4 GiB. Bit
for bit against the sequential model (inflate_oracle.py: CPython's zlib), sentinels around every
region and behind every array, as test_gpu_inflate.py."""
import numpy as np
import pytest

import high_arena as H
import inflate_cases as IC
import inflate_dev_cases as DV
import inflate_oracle as O
from test_gpu_inflate import GAP, Call, T, one_per_connection, place
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def regions(caps, residues):
    """region offsets, region s at an address that is residues[s] mod 16 (the destination itself is
    256-B aligned on the device), GAP sentinel bytes or more between two"""
    offs, at = [], GAP
    for cap, r in zip(caps, residues):
        at += (r - at) % 16
        offs.append(at)
        at += cap + GAP
    return offs


def out_len(body):
    return len(O.inflate_one(body)[1])


def all_ok(c):
    return (c.exp[1]["status"] == O.OK).all()


def test_match_grid_one_message_per_connection(dev):
    grid = DV.match_grid()
    bodies = [g[4] for g in grid]
    src, spans = place(bodies, [(3 * k) % 16 for k in range(len(bodies))])
    caps = [p + ln + 3 + 5 for p, _, ln, _, _ in grid]
    c = Call(dev, src, one_per_connection(spans), caps=caps, offs=regions(caps, [k % 16 for k in range(len(grid))]))
    assert c.dst.data_ptr() % 16 == 0 and {int(o) % 16 for o in c.offs} == set(range(16))
    assert all_ok(c) and [int(v) for v in c.exp[1]["out_len"]] == caps
    c.run()
    c.check("match grid")


@pytest.mark.parametrize("per", [1, 4])
def test_token_streams(dev, per):
    """one stream per connection, and four: the later messages start at whatever address the one
    before ended at, with the run, the wait's position and the window reset"""
    bodies = [b for _, b in DV.token_streams()]
    src, spans = place(bodies, [(5 * k) % 16 for k in range(len(bodies))])
    conns = [[sp + (O.RAW,) for sp in spans[k:k + per]] for k in range(0, len(spans), per)]
    c = Call(dev, src, conns, odd=True)
    assert all_ok(c) and int(c.exp[1]["n_msgs"].sum()) == len(bodies)
    if per > 1:
        assert len({int(r["out_off"]) % 16 for r in c.exp[0]}) == 16
    c.run()
    c.check("token streams, %d per connection" % per)


def test_stored_grid_at_every_source_and_destination_residue(dev):
    """every stored body with its data at source residue a and its output at destination residue b
    for all 256 (a, b) — the two swept independently; the 65,535-byte block at 16 of them"""
    bodies, aligns, dres, sizes = [], [], [], []
    for name, body, n in DV.stored_grid():
        for r in (range(16) if n == 65535 else range(256)):
            a, b = (r % 16, (5 * r + 3) % 16) if n == 65535 else (r % 16, r // 16)
            bodies.append(body)
            aligns.append((a - DV.STORED_DATA_AT) % 16)
            dres.append(b)
            sizes.append(n)
    src, spans = place(bodies, aligns)
    caps = [out_len(b) for b in bodies]
    c = Call(dev, src, one_per_connection(spans), caps=caps, offs=regions(caps, dres))
    assert c.src.data_ptr() % 16 == 0 and c.dst.data_ptr() % 16 == 0
    for n in DV.STORED_PAIRS:
        seen = {((o + DV.STORED_DATA_AT) % 16, int(c.offs[k]) % 16) for k, (o, _) in enumerate(spans) if sizes[k] == n}
        assert len(seen) == 256, n
    assert {O.OK, O.ERR_DATA} == set(int(v) for v in c.exp[1]["status"])
    c.run()
    c.check("stored grid")


def test_window_bodies_at_every_source_alignment(dev):
    bodies = [b for _, b in DV.window_bodies()]
    reps = [(b, (a + 3 * k) % 16) for a in range(16) for k, b in enumerate(bodies)]
    src, spans = place([b for b, _ in reps], [a for _, a in reps])
    for k in range(len(bodies)):
        assert {spans[k + a * len(bodies)][0] % 16 for a in range(16)} == set(range(16))
    c = Call(dev, src, one_per_connection(spans), odd=True)
    c.run()
    c.check("window bodies")


@pytest.fixture(scope="module")
def sweep():
    bodies = IC.random_cases(300, seed=7692)
    assert len(bodies) == 1200
    return (bodies,) + place(bodies, [(7 * k) % 16 for k in range(len(bodies))])


def test_seeded_sweep_as_one_batch(dev, sweep):
    bodies, src, spans = sweep
    c = Call(dev, src, one_per_connection(spans), odd=True)
    st = np.bincount(c.exp[1]["status"], minlength=5)
    assert st[O.OK] >= 600 and st[O.ERR_DATA] >= 200 and st[O.OK] + st[O.ERR_DATA] == 1200
    c.run()
    c.check("sweep")


def test_seeded_sweep_three_to_a_connection_with_a_limit(dev, sweep):
    bodies, src, spans = sweep
    limit = 9000
    conns = [[sp + (O.RAW,) for sp in spans[k:k + 3]] for k in range(0, len(spans), 3)]
    caps, whole = [], bytes(src)
    for s, cn in enumerate(conns):
        need = O.connection(whole, cn, limit, 0, 1 << 40)[1]["out_len"]
        caps.append(max(0, int(need) - 1) if s % 7 == 3 else int(need) + (0 if s % 2 else 11))
    c = Call(dev, src, conns, limit=limit, caps=caps, odd=True)
    seen = set(int(v) for v in c.exp[0]["status"])
    assert seen == {O.OK, O.ERR_DATA, O.ERR_TOO_BIG, O.ERR_OUT_SPACE, O.NOT_RUN}, seen
    c.run()
    c.check("sweep, three to a connection")


# ---------------------------------------------------------------------------------- past 4 GiB

CUT = 1500                                # the destination's 2^32 lies this far into the first message's output


def boundary_stream():
    """a token stream whose output, with 2^32 at byte CUT of it, has a full literal run flushed across
    the boundary and a match whose position lies above it and whose source lies below"""
    rng = np.random.default_rng(32)
    ops = DV.stream_ops(rng, 1150)
    ops += DV.lits(rng, 1465 - len(IC.played(ops))) + [(3, 1)]
    ops += DV.lits(rng, 64 + 2) + [(129, 1000), (258, 40)] + DV.stream_ops(rng, 1200)
    matches, runs = DV.io_trace(ops)
    assert (1468, 64) in runs and 1468 < CUT < 1468 + 64
    assert any(m[:3] == (1534, 1000, 129) for m in matches) and 1534 > CUT > 1534 - 1000 + 129
    assert any(pos > CUT and pos - dist > CUT for pos, dist, _, _, _, _ in matches)
    return ops, IC.fixed_block(ops)


@pytest.fixture(scope="module")
def arenas(dev):
    H.need_memory(torch, pytest)
    a, b = H.Arena(dev), H.Arena(dev)
    yield a, b
    del a.t, b.t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("straddler", ["dynamic", "stored"])
def test_offsets_past_4gib(dev, arenas, straddler):
    """a dynamic body (a window refill) or a stored body (the 16-byte copy) straddles 2^32 in a sparse
    source arena; in a sparse destination arena the first message's output straddles 2^32 and the same
    connection's second message lies wholly above it: results and regions are the oracle's on the small
    images, moved; an offset cut to 31 or 32 bits reads or writes the low aliases (sentinels), and is seen"""
    sa, ta = arenas
    rng = np.random.default_rng(4)
    ops, stream = boundary_stream()
    dyn = IC.deflate(IC.text(rng, 1800) + rng.integers(0, 256, 400, dtype=np.uint8).tobytes() + IC.text(rng, 600), 9)
    sto = IC.deflate(rng.integers(0, 256, 2000, dtype=np.uint8).tobytes(), 0)
    fix = IC.deflate(IC.text(rng, 700), 6, 4)
    assert (dyn[0] >> 1) & 3 == 2 and 900 <= len(dyn) <= 1400 and len(sto) == 2006
    small, spans = place([stream, dyn, sto, fix], [3, 9, 6, 1])
    at = spans[1][0] + 500 if straddler == "dynamic" else spans[2][0] + DV.STORED_DATA_AT + 1003
    high = H.place(H.B32, at)                             # this source byte lies at 2^32
    conns = [[spans[0] + (O.RAW,), spans[1] + (O.RAW,)], [spans[2] + (O.RAW,), spans[3] + (O.RAW,)]]
    mm, nseg = 2, 2
    msg = np.array([e + (0,) for cn in conns for e in cn], O.MSG_DTYPE)
    nmsg = np.array([2, 2], np.uint32)
    caps = np.array([out_len(stream) + out_len(dyn), 2000 + 700], np.uint64)
    offs = np.array([64, 64 + int(caps[0]) + 37], np.uint64)
    dlen = int(offs[1] + caps[1]) + 64
    emr, eres, outs = O.batch(small, msg, nmsg, mm, 0, offs, caps, fill=O.FILL)
    assert (eres["status"] == O.OK).all() and outs[0][:len(IC.played(ops))] == IC.played(ops)
    edst = np.full(dlen, O.FILL, np.uint8)
    for s in range(nseg):
        edst[int(offs[s]):int(offs[s]) + len(outs[s])] = np.frombuffer(outs[s], np.uint8)
    dhigh = H.place(H.B32, 64 + CUT)                      # byte CUT of the first message's output lies at 2^32
    assert int(emr[1]["out_off"]) + dhigh > H.B32 and int(emr[0]["out_off"]) + dhigh < H.B32
    placed_src = sa.put(high, small)
    placed_dst = ta.put(dhigh, np.full(dlen, O.FILL, np.uint8))
    hm = msg.copy()
    hm["src_off"] += np.uint64(high)
    mres = torch.full((24 * nseg * mm + 24,), O.FILL, dtype=torch.uint8, device=dev)
    res = torch.full((24 * nseg + 24,), O.FILL, dtype=torch.uint8, device=dev)
    W.batch_inflate_device(sa.view(high, len(small)), T(hm, dev), T(nmsg, dev).view(torch.int32), mm, ta.view(dhigh, dlen),
                           T(offs + np.uint64(dhigh), dev).view(torch.int64), T(caps, dev).view(torch.int64),
                           mres[:24 * nseg * mm], res[:24 * nseg], src_len=high + len(small))
    torch.cuda.synchronize()
    want = emr.copy()
    want["out_off"] += np.uint64(dhigh)
    gm, gr = mres.cpu().numpy(), res.cpu().numpy()
    assert np.array_equal(gm[:24 * nseg * mm].view(O.MSGRES_DTYPE), want), (gm[:24 * nseg * mm].view(O.MSGRES_DTYPE), want)
    assert np.array_equal(gr[:24 * nseg].view(O.RES_DTYPE), eres), (gr[:24 * nseg].view(O.RES_DTYPE), eres)
    assert (gm[24 * nseg * mm:] == O.FILL).all() and (gr[24 * nseg:] == O.FILL).all()
    ta.check(placed_dst, edst, "regions past 2^32")
    sa.check(placed_src, small, "source past 2^32")
