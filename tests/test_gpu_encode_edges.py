"""GPU parity of websocketframeBatchEncodeDevice at the geometries where its three store
mechanisms (copy kernel, shift path, byte path) hand over to each other: every destination
phase, headers across piece and wave-range boundaries, the record-load switch points, frame
counts around the scan tiles, every capacity cut, extended type / flag bytes and 64-bit
lengths, source and wire offsets. The expected bytes and offsets always come from
enc_cases.encode_ref (pinned to the oracle in tests/test_enc_cases.py); every byte of the
destination buffer is compared, the 0xA5 sentinels around and past the output included."""
import ctypes as C

import numpy as np
import pytest

import enc_cases as E
from oracle_lib import load_oracle
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SLACK = 64                          # sentinel bytes on each side of the destination
FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def release_device_memory(dev):
    """set up first, so torn down last: the cached cases and the 4 GiB source go back to the
    device before the next module runs, with nothing of this one still in flight"""
    yield
    import gc
    Case.cache.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True, params=[1, 0], ids=["front", "hipcub"])
def front(request, dev):
    """every test runs on both fronts: F1-F3 (tile scan + per-frame offsets, piece pointers
    and edge chunks before E3) and hipcub scan + E2, E3, E4"""
    W.set_option("enc_front", request.param)
    yield request.param
    W.set_option("enc_front", 1)


class Case:
    """one batch on the device with its reference output (computed once, shared by both fronts)"""
    cache = {}

    def __init__(self, dev, src, fr):
        self.fr = fr
        self.n = len(fr)
        self.want, self.woff = E.encode_ref(src, fr)
        self.total = len(self.want)
        self.src_t = torch.from_numpy(src).to(dev)
        self.fr_t = torch.from_numpy(fr.view(np.uint8).copy()).to(dev)
        self.want_t = torch.from_numpy(self.want).to(dev)
        self.woff_t = torch.from_numpy(self.woff.astype(np.int64)).to(dev)
        self.off_t = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)

    @classmethod
    def get(cls, dev, key, build):
        if key not in cls.cache:
            cls.cache[key] = Case(dev, *build())
        return cls.cache[key]

    def buffers(self, shift, max_cap=None):
        size = SLACK + shift + max(self.total, max_cap or 0) + SLACK
        dev = self.src_t.device
        return torch.empty(size, dtype=torch.uint8, device=dev), torch.empty(size, dtype=torch.uint8, device=dev)

    def run(self, shift, cap=None, bufs=None, tag=""):
        """encode to a destination of phase `shift` with `cap` bytes of capacity (default: the
        wire size) and compare the whole buffer and the offsets with the reference"""
        cap = self.total if cap is None else cap
        out, exp = bufs if bufs is not None else self.buffers(shift, cap)
        dst = out[SLACK + shift:]
        assert dst.data_ptr() & 15 == shift & 15 and dst.numel() >= cap + SLACK
        out.fill_(FILL)
        self.off_t.fill_(-1)
        W.batch_encode_device(self.src_t, self.fr_t, dst, self.off_t, capacity=cap)
        w = min(self.total, cap)
        exp.fill_(FILL)
        exp[SLACK + shift:SLACK + shift + w].copy_(self.want_t[:w])
        if not torch.equal(self.off_t, self.woff_t):
            got = self.off_t.cpu().numpy().astype(np.uint64)
            bad = int(np.nonzero(got != self.woff)[0][0])
            raise AssertionError("%s shift %d cap %d: wire_off[%d] = %d, want %d"
                                 % (tag, shift, cap, bad, int(got[bad]), int(self.woff[bad])))
        if not torch.equal(out, exp):
            self.report(out.cpu().numpy(), exp.cpu().numpy(), shift, cap, tag)

    def report(self, got, exp, shift, cap, tag):
        bad = np.nonzero(got != exp)[0]
        p = int(bad[0]) - SLACK - shift                                  # dst-relative
        i = min(max(E.frame_at(self.woff, max(p, 0)), 0), self.n - 1)
        row = E.classify(self.fr, shift & 15, cap)[i]
        where = "before dst" if p < 0 else ("past the output" if p >= min(self.total, cap) else "inside the output")
        raise AssertionError(
            "%s shift %d cap %d (wire %d): %d bytes differ, first at dst offset %d (%s): got 0x%02x, want 0x%02x; "
            "frame %d at wire offset %d, len %d: %s"
            % (tag, shift, cap, self.total, len(bad), p, where, int(got[bad[0]]), int(exp[bad[0]]), i,
               int(self.woff[i]), int(self.fr["len"][i]), dict(zip(row.dtype.names, (int(x) for x in row)))))


@pytest.mark.parametrize("shift", range(16))
def test_chain_every_dst_phase(dev, shift):
    """the chains (every edge geometry, tests/test_enc_cases.py::test_chain_coverage) at each of
    the 16 destination phases: frame 0's eligibility and the partial first chunk"""
    for seed in (1, 2):
        Case.get(dev, ("chain", seed), lambda: E.chain(seed)).run(shift, tag="chain(%d)" % seed)


def test_header_straddles_piece_and_wave_boundaries(dev):
    """headers of all six lengths split at every byte over a piece boundary (16384) and over
    the wave-range boundaries 4096 and 12288, the filler rebuilt for the destination phase"""
    for shift in (0, 7):
        for case in E.STRADDLE_CASES:
            c = Case.get(dev, ("straddle", case, shift), lambda: E.straddle(*case, lead0=shift))
            assert int(c.woff[1]) + shift == case[0] - case[2]
            c.run(shift, tag="straddle%r" % (case,))


@pytest.mark.parametrize("m", E.PER_PIECE_M)
def test_frames_per_piece_switch_points(dev, m):
    """m frames touching one piece / one wave range: the copy kernel's record loop loads
    exactly the piece's frames up to 16 of them, else 16 and then 64 at a time"""
    for shift in (0, 7):
        Case.get(dev, ("piece", m, shift), lambda: E.per_piece(m, lead0=shift)).run(shift, tag="per_piece(%d)" % m)
        Case.get(dev, ("wave", m, shift), lambda: E.per_wave(m, lead0=shift)).run(shift, tag="per_wave(%d)" % m)


@pytest.mark.parametrize("n", E.COUNTS_N)
def test_frame_count_edges(dev, n):
    """1, 2 and one tile +- 1 frames; 1024 / 1025 / 2049 tiles (the tile scan's per-thread count
    goes 1 -> 2 -> 3)"""
    c = Case.get(dev, ("counts", n), lambda: E.counts(n))
    for shift in (0, 11):
        c.run(shift, tag="counts(%d)" % n)


@pytest.mark.parametrize("shift", [0, 1, 9, 15])
def test_capacity_every_cut(dev, shift):
    """every capacity from 0 to past the wire on a 14-frame batch (2/4/6/8-byte headers); on a
    batch with the 10/14-byte headers, which need 64 KiB payloads, every capacity within 20
    bytes of each frame's start, payload start and end; and around the first piece boundary.
    Offsets exact, output exact up to the cut, nothing written past it."""
    c = Case.get(dev, "cap", E.capacity_batch)
    bufs = c.buffers(shift, c.total + 17)
    for cap in range(c.total + 18):
        c.run(shift, cap, bufs, tag="capacity_batch")
    c = Case.get(dev, "cap_long", E.capacity_batch_long)
    bufs = c.buffers(shift, c.total + 20)
    for cap in E.capacity_cuts_long(c.fr):
        c.run(shift, cap, bufs, tag="capacity_batch_long")
    c = Case.get(dev, ("cap_boundary", shift), lambda: E.capacity_boundary_batch(shift))
    bufs = c.buffers(shift)
    for cap in range(E.PIECE - shift - 40, E.PIECE - shift + 41):
        c.run(shift, cap, bufs, tag="capacity_boundary_batch")


def test_capacity_zero_and_oversized(dev):
    """capacity 0: only the offsets are written; a capacity three pieces past the wire: the
    trailing pieces stay untouched"""
    for shift in (0, 5):
        for key, build in (("cap", E.capacity_batch), (("cap_boundary", shift), lambda: E.capacity_boundary_batch(shift)),
                           (("chain", 1), lambda: E.chain(1))):
            c = Case.get(dev, key, build)
            c.run(shift, 0, tag="%r capacity 0" % (key,))
            c.run(shift, c.total + 3 * E.PIECE, tag="%r oversized" % (key,))
            c.run(shift, c.total + 3 * E.PIECE + 5, tag="%r oversized" % (key,))


def test_extended_type_and_flag_bytes(dev):
    """type 0..255 and is_fin / prev_is_fin / masked in {0, 1, 2, 255}: the reference takes
    ints, tests them for non-zero and stores type | 0x80 into a byte (websocketframe.c:176-189)"""
    c = Case.get(dev, "flags", E.flag_batch)
    for shift in (0, 6):
        c.run(shift, tag="flag_batch")


# ---- 64-bit lengths, source offsets and wire offsets

BIG_LEN = (1 << 32) + 5
BIG_SRC = (1 << 32) + (1 << 20)
SLICE = 1 << 28


@pytest.fixture(scope="module")
def big_src(dev):
    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip("a 2^32 + 5 byte frame needs 12 GiB of free device memory (src, dst, compare slices): %.1f GiB free"
                    % (free / 2**30))
    s = torch.empty(BIG_SRC, dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(64)
    for a in range(0, BIG_SRC, SLICE):                                   # filled on the device, never copied
        b = min(a + SLICE, BIG_SRC)
        s[a:b] = torch.randint(0, 256, (b - a,), dtype=torch.uint8, device=dev, generator=g)
    yield s
    del s                                                                # release_device_memory empties the cache


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("masked", [1, 0], ids=["masked", "unmasked"])
def test_64bit_len_src_and_wire_offsets(dev, big_src, masked, shift):
    """one frame of 2^32 + 5 payload bytes after 3 short frames, and 6 short frames after it
    whose source and wire offsets are >= 2^32: the high bytes of the 64-bit length header, the
    two-half lane reads of src / len / off and the 64-bit piece offsets. The big header comes
    from the oracle (+ MASK bit and key), the short frames from encode_ref on host copies of
    their source bytes; the big payload is compared on the device in 256 MiB slices."""
    rng = np.random.default_rng(640 + masked)
    rows = [(100, 3, 1), (1000, 40, 0), (5000, 130, 1),
            (7, BIG_LEN, masked),
            ((1 << 32) + 16, 0, 1), ((1 << 32) + 100, 5, 0), ((1 << 32) + 1001, 40, 1), ((1 << 32) + 5003, 200, 1),
            ((1 << 32) + 9000, 126, 0), ((1 << 32) + 200005, 70001, 1)]
    fr = np.zeros(len(rows), W.ENC_DTYPE)
    for i, (so, ln, m) in enumerate(rows):
        fr[i] = (so, ln, int(rng.integers(1, 2**32)), int(rng.integers(0, 256)), int(rng.choice(E.FLAGS)),
                 int(rng.choice(E.FLAGS)), m)
    big = 3
    # the short frames against host copies of their source bytes
    small = [i for i in range(len(fr)) if i != big]
    host_src = np.concatenate([big_src[int(fr[i]["src_off"]):int(fr[i]["src_off"] + fr[i]["len"])].cpu().numpy()
                               for i in small] + [np.zeros(E.SRC_SLACK, np.uint8)])
    hfr = fr[small].copy()
    hfr["src_off"] = np.cumsum(np.append(0, hfr["len"][:-1]))
    pre, pre_off = E.encode_ref(host_src, hfr[:big])
    post, post_off = E.encode_ref(host_src, hfr[big:])
    lib = load_oracle()
    hb = (C.c_ubyte * 10)()
    assert lib.ws_oracle_encode_headlen(BIG_LEN) == 10
    lib.ws_oracle_encode(hb, int(fr[big]["is_fin"]), int(fr[big]["prev_is_fin"]), int(fr[big]["type"]), BIG_LEN)
    hdr = bytearray(bytes(hb))
    key = int(fr[big]["mask_key"]).to_bytes(4, "little")
    if masked:
        hdr[1] |= 0x80
        hdr += key
    d0 = len(pre) + len(hdr)                                             # the big payload, dst-relative
    d1 = d0 + BIG_LEN
    total = d1 + len(post)
    woff = np.concatenate([pre_off[:-1], np.array([len(pre)], np.uint64), post_off + np.uint64(d1)])
    assert int(woff[big + 1]) >= 1 << 32 and int(woff[-1]) == total

    f_t = torch.from_numpy(fr.view(np.uint8).copy()).to(dev)
    off_t = torch.full((len(fr) + 1,), -1, dtype=torch.int64, device=dev)
    out = torch.empty(SLACK + shift + total + SLACK, dtype=torch.uint8, device=dev)
    base = SLACK + shift
    out[:base + d0 + 4096].fill_(FILL)                                   # the big payload region is compared in full,
    out[base + d1 - 4096:].fill_(FILL)                                   # so only its surroundings need the sentinel
    dst = out[base:]
    assert dst.data_ptr() & 15 == shift
    W.batch_encode_device(big_src, f_t, dst, off_t, capacity=total)
    torch.cuda.synchronize()

    assert np.array_equal(off_t.cpu().numpy().astype(np.uint64), woff)
    sent = np.full(SLACK + shift, FILL, np.uint8)
    head = np.concatenate([sent, pre, np.frombuffer(bytes(hdr), dtype=np.uint8)])
    got_head = out[:base + d0].cpu().numpy()
    assert np.array_equal(got_head, head), "first difference at dst offset %d" % (
        int(np.nonzero(got_head != head)[0][0]) - base)
    tail = np.concatenate([post, np.full(SLACK, FILL, np.uint8)])
    got_tail = out[base + d1:].cpu().numpy()
    assert np.array_equal(got_tail, tail), "first difference %d bytes past the big payload" % (
        int(np.nonzero(got_tail != tail)[0][0]))
    key_tile = torch.from_numpy(np.frombuffer(key if masked else bytes(4), dtype=np.uint8).copy()).to(dev).repeat(SLICE // 4)
    so = int(fr[big]["src_off"])
    for a in range(0, BIG_LEN, SLICE):                                   # SLICE % 4 == 0: the key phase restarts
        b = min(a + SLICE, BIG_LEN)
        same = (out[base + d0 + a:base + d0 + b] == (big_src[so + a:so + b] ^ key_tile[:b - a])).all()
        assert bool(same), "big payload differs in bytes [%d, %d)" % (a, b)
    del out, key_tile
