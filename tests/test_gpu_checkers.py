"""The device checkers every full-size test leans on must be able to fail: Workload.verify
(ws_verify_kernel) counts exactly the payload bytes that differ, in the second grid-stride round
and in a partial last word as well, and reads no header and no pad byte; the ranged generator
equals the numpy one; Workload.check_descs raises for one changed field of one slot, whichever;
Workload.output_hash (ws_hash_kernel) moves with one payload byte, one descriptor field or one
frame count, and equals its numpy statement on a batch whose data_off are 2^32 and more."""
import numpy as np
import pytest

import bench
import high_arena as H
import wsynth
from oracle_lib import oracle_segments
from util_amd import dist
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROUND = 65536                        # blocks of the synth and verify kernels: frames past it take a second round


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def release_device_memory(dev):
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def payload_pos(wl, f, b):
    """buffer offset of payload byte b (negative: from the end) of frame f"""
    plen = int(wl.plen_h[f])
    return int(wl.off_h[f]) + int(wl.wirelen_h[f]) - plen + (b if b >= 0 else plen + b)


def flip(t, positions):
    for p in positions:
        t[p] ^= 0x01


WORKLOADS = {"cfg2_70000": ("cfg2", dict(nframes=70000)), "cfg3_70000": ("cfg3", dict(nframes=70000)),
             "plen1001": ("cfg2", dict(nframes=4096, plen=1001))}


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_verify_counts_every_flipped_payload_byte(dev, name):
    cfg, kw = WORKLOADS[name]
    wl = bench.Workload.make(cfg, dev, **kw)
    try:
        n = wl.nframes
        assert wl.verify(False) == 0
        wl.decode()
        torch.cuda.synchronize()
        assert wl.verify(True) == 0
        spots = {"payload byte 0 of frame 0": payload_pos(wl, 0, 0),
                 "the last payload byte of the last frame": payload_pos(wl, n - 1, -1)}
        partial = [f for f in range(min(n, 4096)) if int(wl.plen_h[f]) % 8]
        if name != "cfg2_70000":                            # 4096-byte payloads have no partial word
            spots["the last byte of a partial word"] = payload_pos(wl, partial[len(partial) // 2], -1)
        if n > ROUND:
            spots["a byte of a frame in the second round"] = payload_pos(wl, ROUND + 1234, 7)
        else:
            assert name == "plen1001"
        for what, p in spots.items():
            flip(wl.buf, [p])
            got = wl.verify(True)
            flip(wl.buf, [p])
            assert got == 1, (what, got)
        assert wl.verify(True) == 0
        many = [payload_pos(wl, f, (f * 7) % int(wl.plen_h[f])) for f in (1, 2, n // 3, n // 2, n - 2)]
        many += [many[0] + 1, many[0] + 2]                   # three in one frame, two of them in one word
        flip(wl.buf, many)
        got = wl.verify(True)
        flip(wl.buf, many)
        assert got == len(many) == 7, got
        # the documented limit: verify reads payloads only
        blind = [int(wl.off_h[3]) + 1, int(wl.off_h[n - 1]), wl.wire_bytes + 10]
        flip(wl.buf, blind)
        got = wl.verify(True)
        flip(wl.buf, blind)
        assert got == 0, "verify counted a header or a pad byte"
        assert wl.verify(True) == 0
    finally:
        wl.free()


@pytest.mark.parametrize("cfg,pk,fl,bk,seed", [("cfg3", wsynth.PLEN_MIX3, 0, wsynth.B0_BINARY, 3),
                                               ("cfg5", wsynth.PLEN_FIXED, 1024, wsynth.B0_FRAG16, 5),
                                               ("cfg1", wsynth.PLEN_FIXED, 125, wsynth.B0_TEXT, 1)])
def test_generator_range_equals_numpy(dev, cfg, pk, fl, bk, seed):
    wl = bench.Workload.make(cfg, dev, nframes=304, first_frame=12345)
    wire, off, pl, plain = wsynth.make_batch(304, pk, fl, bk, seed, first=12345)
    assert wl.wire_bytes == len(wire) and np.array_equal(wl.off_h, off)
    assert np.array_equal(wl.buf[:len(wire)].cpu().numpy(), wire)
    assert wl.verify(False) == 0
    wl.decode()
    torch.cuda.synchronize()
    assert np.array_equal(wl.buf[:len(wire)].cpu().numpy(), plain)
    assert wl.verify(True) == 0
    wl.check_descs()
    wl.free()


def test_verify_with_first_frame_off_by_one(dev):
    """frames of one length, so the frame offsets hold and only keys and payloads move"""
    wl = bench.Workload.make("cfg2", dev, nframes=304, plen=1001, first_frame=12345)
    assert wl.verify(False) == 0
    for d in (1, -1):
        wl.first_frame = 12345 + d
        assert wl.verify(False) > 304 * 900, d
    wl.first_frame = 12345
    assert wl.verify(False) == 0
    wl.free()


DESC_FIELDS = {"frame_off": 0, "frame_off high half": 5, "data_off": 8, "data_off high half": 12, "datalen": 16,
               "datalen high half": 21, "ret": 24, "ret high byte": 27, "is_fin": 28, "type": 29, "masked": 30, "hdrlen": 31}


@pytest.mark.parametrize("cfg", ["cfg3", "cfg5"])
def test_check_descs_raises_for_any_changed_field(dev, cfg):
    wl = bench.Workload.make(cfg, dev, nframes=4096)
    assert wl.b0_kind == (2 if cfg == "cfg5" else 0)
    try:
        wl.decode()
        torch.cuda.synchronize()
        wl.check_descs()
        for slot in (0, 2049, 4095):
            for field, at in DESC_FIELDS.items():
                wl.desc[slot * 32 + at] ^= 0x01
                with pytest.raises(AssertionError):
                    wl.check_descs()
                wl.desc[slot * 32 + at] ^= 0x01
        wl.check_descs()
    finally:
        wl.free()


def test_output_hash_moves_with_every_input(dev):
    wl = bench.Workload.make("cfg3", dev, nframes=4096)
    try:
        wl.decode()
        torch.cuda.synchronize()
        h0 = wl.output_hash()
        assert h0 != 0 and wl.output_hash() == h0
        seen = {h0}
        for what, t, p in (("first payload byte", wl.buf, payload_pos(wl, 0, 0)),
                           ("last payload byte", wl.buf, payload_pos(wl, 4095, -1)),
                           ("a payload byte in the middle", wl.buf, payload_pos(wl, 2000, 77)),
                           ("datalen", wl.desc, 1000 * 32 + 16), ("is_fin", wl.desc, 1001 * 32 + 28),
                           ("type", wl.desc, 1002 * 32 + 29), ("n_frames", wl.res, 5 * 16 + 8)):
            was = int(t[p])
            t[p] = was - 1 if what == "n_frames" else was ^ 0x01       # 16 frames -> 15: one fewer
            h = wl.output_hash()
            t[p] = was
            assert h not in seen, what
            seen.add(h)
        assert wl.output_hash() == h0
    finally:
        wl.free()


def test_device_hash_equals_numpy_at_high_data_off(dev):
    """ws_hash_kernel against util_amd/dist.py:batch_hash on the byte-exact batch decoded by the
    oracle and placed wholly above 2^32 and across it: every data_off handed in is HIGH + the oracle's"""
    H.need_memory(torch, pytest)
    arena = H.Arena(dev)
    try:
        wire, so, sl, mf, at = H.byte_exact()
        img = wire.copy()
        od, orr = oracle_segments(img, so, sl, mf)
        want = dist.batch_hash(img, od, orr, mf)
        assert want != 0
        for high in (H.ABOVE, H.place(H.B32, at["payload_mid_chunk"]), H.place(H.B33, at["payload_first"])):
            placed = arena.put(high, img)
            up = H.rebase(od, high)
            assert (up["data_off"][:1] >= np.uint64(H.B31)).all()
            desc = arena.up(up.view(np.uint8).copy())
            res = arena.up(orr.view(np.uint8).copy())
            h = torch.zeros(1, dtype=torch.int64, device=dev)
            W.frame_hash_device(arena.view(high, len(img)), desc, res, len(so), mf, h)
            torch.cuda.synchronize()
            assert (int(h.item()) & 0xFFFFFFFFFFFFFFFF) == want, hex(high)
            arena.check(placed, img, "hash at 0x%x" % high)
    finally:
        del arena.t
        torch.cuda.empty_cache()
