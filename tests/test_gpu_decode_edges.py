"""GPU parity of websocketframeBatchDecodeDevice on the directed batches of tests/dec_cases.py:
runs of equal frames with every ending and every max_frames around them, alphabet patterns cut at
every byte, headers split over piece boundaries and segfuse window edges, small payloads at every
chunk phase, dense items, long frames that are not first, on all four decode paths, at base
addresses of every 16-byte phase. The whole allocation is compared with the oracle's image: the
bytes before the buffer, the 0xA5 gaps and the pad must come back untouched, results and used
descriptors equal the oracle's, unused descriptor slots keep their fill."""
import numpy as np
import pytest

import dec_cases as D
from oracle_lib import oracle_segments
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PREFIX, PAD = 64, 64
PRE_FILL, PAD_FILL, SLOT_FILL = 0x5C, 0x3C, 0xEE
CATALOGUE = {cid: (fn, kw, mfs) for cid, fn, kw, mfs in D.catalogue()}
IDS = list(CATALOGUE)

_wire, _want = {}, {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def release_device_memory(dev):
    """set up first, so torn down last: nothing of this module stays on the device"""
    yield
    import gc
    _wire.clear()
    _want.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def case(cid, shift):
    key = (cid, shift if cid.split(":")[0] in D.GEOMETRIC else 0)
    if key not in _wire:
        fn, kw, _ = CATALOGUE[cid]
        _wire[key] = fn(key[1], **kw)[:3]
    return key, _wire[key]


def want(cid, shift, mf):
    """(oracle image, descriptor bytes with unused slots at their fill, results), computed once"""
    key, (wire, so, sl) = case(cid, shift)
    if key + (mf,) not in _want:
        img = wire.copy()
        od, orr = oracle_segments(img, so, sl, mf)
        nseg = len(so)
        dimg = np.full((max(1, nseg * mf), 32), SLOT_FILL, np.uint8)
        used = (np.arange(mf)[None, :] < orr["n_frames"][:, None]).reshape(-1)
        dimg[:nseg * mf][used] = od[:nseg * mf].view(np.uint8).reshape(-1, 32)[used]
        _want[key + (mf,)] = (img, dimg, orr.copy())
    return (wire, so, sl) + _want[key + (mf,)]


class Loaded:
    """one case at one base shift on the device: [64 x 0x5C | shift x 0x5C | wire | 64 x 0x3C]"""

    def __init__(self, dev, cid, shift, mf, perm=None):
        wire, so, sl, img, dimg, orr = want(cid, shift, mf)
        self.tag = "%s shift %d max_frames %d%s" % (cid, shift, mf, "" if perm is None else " permuted")
        self.n, self.shift, self.mf, self.nseg = len(wire), shift, mf, len(so)
        if perm is not None:
            so, sl = [so[i] for i in perm], [sl[i] for i in perm]
            orr = orr[perm]
            dimg = dimg.reshape(self.nseg, mf, 32)[perm].reshape(-1, 32)
        pre, pad = np.full(PREFIX + shift, PRE_FILL, np.uint8), np.full(PAD, PAD_FILL, np.uint8)
        self.pristine = torch.from_numpy(np.concatenate([pre, wire, pad])).to(dev)
        self.exp = torch.from_numpy(np.concatenate([pre, img, pad])).to(dev)
        self.buf = torch.empty_like(self.pristine)
        self.view = self.buf[PREFIX + shift:]
        assert self.view.data_ptr() & 15 == shift
        self.so = torch.tensor(np.asarray(so, dtype=np.int64), device=dev)
        self.sl = torch.tensor(np.asarray(sl, dtype=np.int64), device=dev)
        # one segment's worth of spare slots after the last: a frame taken past max_frames lands there
        dimg = np.concatenate([dimg, np.full((mf, 32), SLOT_FILL, np.uint8)])
        self.exp_desc = torch.from_numpy(dimg.reshape(-1).copy()).to(dev)
        self.exp_res = torch.from_numpy(orr.view(np.uint8).copy()).to(dev)
        self.desc = torch.empty_like(self.exp_desc)
        self.res = torch.empty(max(1, self.nseg) * 16, dtype=torch.uint8, device=dev)

    def run(self, what=""):
        self.buf.copy_(self.pristine)
        self.desc.fill_(SLOT_FILL)
        self.res.fill_(SLOT_FILL)
        W.batch_decode_device(self.view, self.so, self.sl, self.mf, self.desc, self.res)
        tag = self.tag + " " + what
        if not torch.equal(self.res[:self.nseg * 16], self.exp_res):
            g = self.res[:self.nseg * 16].cpu().numpy().view(W.SEGRES_DTYPE)
            e = self.exp_res.cpu().numpy().view(W.SEGRES_DTYPE)
            s = int(np.nonzero(g != e)[0][0])
            raise AssertionError("%s: result of segment %d is %s, want %s" % (tag, s, g[s], e[s]))
        if not torch.equal(self.desc, self.exp_desc):
            g, e = self.desc.cpu().numpy().reshape(-1, 32), self.exp_desc.cpu().numpy().reshape(-1, 32)
            i = int(np.nonzero((g != e).any(axis=1))[0][0])
            raise AssertionError("%s: descriptor slot %d (segment %d, frame %d) is %s, want %s (0xEE: unused)"
                                 % (tag, i, i // self.mf, i % self.mf, g[i].copy().view(W.DESC_DTYPE)[0],
                                    e[i].copy().view(W.DESC_DTYPE)[0]))
        if not torch.equal(self.buf, self.exp):
            g, e = self.buf.cpu().numpy(), self.exp.cpu().numpy()
            bad = np.nonzero(g != e)[0]
            p = int(bad[0]) - PREFIX - self.shift
            zone = "before the buffer" if p < 0 else ("in the pad" if p >= self.n else "inside the batch")
            raise AssertionError("%s: %d bytes differ, first at buffer offset %d (%s): got 0x%02x, want 0x%02x (wire 0x%02x)"
                                 % (tag, len(bad), p, zone, int(g[bad[0]]), int(e[bad[0]]),
                                    int(self.pristine[bad[0]].item())))


def paths_for(mf):
    """3 piece, 4 segfuse, 1 walker, -1 auto; path 4 silently becomes 3 above 64 frames: not run twice"""
    return [p for p in (3, 4, 1, -1) if not (p == 4 and mf > 64)]


PATH_IDS = {3: "piece", 4: "segfuse", 1: "walker", -1: "auto"}


@pytest.mark.parametrize("cid,path", [pytest.param(c, p, id="%s-%s" % (c, PATH_IDS[p])) for c in IDS for p in PATH_IDS
                                      if any(p in paths_for(mf) for mf in CATALOGUE[c][2])])
def test_directed_case(dev, cid, path):
    """every max_frames of the case at every base shift, twice in a row on one stream: the second
    call runs with the stride hint and the window advice of the first"""
    W.set_option("path", path)
    try:
        for shift in D.shifts_of(cid):
            for mf in CATALOGUE[cid][2]:
                if path not in paths_for(mf):
                    continue
                c = Loaded(dev, cid, shift, mf)
                c.run("first call")
                c.run("second call")
    finally:
        W.set_option("path", -1)


@pytest.mark.parametrize("cid", [c for c in IDS if c not in ("dense_items:frames", "dense_items:frames64")])   # one segment
def test_permuted_segments_take_the_fallback_walker(dev, cid):
    """segments out of buffer order: K1 marks the batch, K2 stores nothing and walks it"""
    W.set_option("path", 3)
    try:
        for shift in (0, 15):
            mf = CATALOGUE[cid][2][0]
            nseg = len(case(cid, shift)[1][1])
            perm = np.random.default_rng(nseg).permutation(nseg)
            if (np.diff(perm) > 0).all():
                perm = perm[::-1].copy()
            c = Loaded(dev, cid, shift, mf, perm=perm)
            c.run("first call")
            c.run("second call")
    finally:
        W.set_option("path", -1)


@pytest.mark.parametrize("pattern", list(D.PATTERNS))
def test_alphabets_by_stride_speculation_only(dev, pattern):
    """scan_alpha 0: K1 never enters alphabet speculation; same results"""
    W.set_option("path", 3)
    W.set_option("scan_alpha", 0)
    try:
        for variant in ("full", "sweep"):
            cid = "alphabets:%s:%s" % (pattern, variant)
            for shift in D.shifts_of(cid):
                for mf in CATALOGUE[cid][2]:
                    c = Loaded(dev, cid, shift, mf)
                    c.run("scan_alpha 0, first call")
                    c.run("scan_alpha 0, second call")
    finally:
        W.set_option("scan_alpha", 1)
        W.set_option("path", -1)


REASM_IDS = [c for c in IDS if c.split(":")[0] in ("run_lengths", "alphabets") or c in ("dense_items:frames64",
                                                                                       "dense_items:segments")]


@pytest.mark.parametrize("reasm_path", [1, 2], ids=["fused", "three_kernel"])
@pytest.mark.parametrize("cid", REASM_IDS)
def test_reassembly_shares_the_walk(dev, cid, reasm_path):
    """the reassembly's three-kernel path runs K1 too, the fused one the segfuse walk"""
    from test_gpu_reasm import check
    W.set_option("reasm_path", reasm_path)
    try:
        for mf in CATALOGUE[cid][2]:
            wire, so, sl = case(cid, 0)[1]
            check(dev, wire, so, sl, mf, tag="%s max_frames %d reasm_path %d" % (cid, mf, reasm_path))
    finally:
        W.set_option("reasm_path", 0)
