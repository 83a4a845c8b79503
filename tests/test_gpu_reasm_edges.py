"""GPU parity of websocketframeBatchReassembleDevice(Ex/Ctl) on the directed batches of
tests/reasm_dir_cases.py: headers, payload starts and body ends at the fused kernel's window edges
in its first three windows, every source phase x destination phase x length of the body copy,
control bodies packed downward, events on the first and last lane of a walk round, carried
messages (u32 cached bytes included), permuted and empty segments, and the dispatch rule at its
thresholds. Every case runs on the fused kernel in its three geometries, on the three-kernel path
and as dispatched by default, with and without WEBSOCKET_REASM_CONTROL_DIRECT, at two base phases
of the wire and output buffers, bit-exact against the oracle through the check helpers of
test_gpu_reasm.py and test_gpu_reasm_ctl.py: descriptors, segment results, message descriptors,
bodies, d_open, d_cached, the wire untouched, and 0xEE in every output byte outside the bodies."""
import numpy as np
import pytest

import reasm_dir_cases as D
import test_gpu_reasm as P
import test_gpu_reasm_ctl as C
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CATALOGUE = {cid: (fn, kw, mfs) for cid, fn, kw, mfs in D.catalogue()}
# (reasm_path, reasm_cfg); a fused configuration takes the three-kernel path above 64 frames
CONFIGS = {"fused_cfg0": (1, 0), "fused_cfg1": (1, 1), "fused_cfg2": (1, 2), "three_kernel": (2, 0), "auto": (0, 0)}

_case, _oracle = {}, {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def release(dev):
    yield
    _case.clear()
    _oracle.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def case(cid, base):
    if (cid, base) not in _case:
        fn, kw, _ = CATALOGUE[cid]
        _case[cid, base] = fn(bw=base[0], bo=base[1], **kw)
    return _case[cid, base]


def oracle(cid, base, mf, flags):
    """computed once per case, shared by the five configurations, never modified"""
    key = (cid, base, mf, flags)
    if key not in _oracle:
        _oracle[key] = D.oracle(case(cid, base), mf, flags)
    return _oracle[key]


def run(dev, c, mf, base, flags, orc, tag, buflen=None):
    wire, so, sl, _, kw = c
    args = dict(open_in=kw["open_in"], out_off=kw["out_off"], out_size=kw["out_size"], readcache_max=kw["readcache_max"],
                cached_in=kw["cached_in"], shift=base[0], out_shift=base[1], buflen=buflen, oracle=orc, tag=tag)
    if flags:
        C.check(dev, wire, so, sl, mf, **args)             # compares every output byte, the fill included
    else:
        P.check(dev, wire, so, sl, mf, fill=True, **args)


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("cid", list(CATALOGUE))
def test_directed_case(dev, cid, config):
    path, cfg = CONFIGS[config]
    W.set_option("reasm_path", path)
    W.set_option("reasm_cfg", cfg)
    try:
        for base in D.BASES:
            for mf in CATALOGUE[cid][2]:
                for flags in (0, D.CTL):
                    tag = "%s %s max_frames %d base %s flags %d" % (cid, config, mf, base, flags)
                    run(dev, case(cid, base), mf, base, flags, oracle(cid, base, mf, flags), tag)
    finally:
        W.set_option("reasm_cfg", 0)
        W.set_option("reasm_path", 0)


@pytest.mark.parametrize("nseg,mf,plus", D.AUTO_CORNERS)
def test_auto_rule_corners(dev, nseg, mf, plus):
    """reasm_path 0 as shipped, buflen passed explicitly: max_frames <= 64 && nseg >= 1024 &&
    buflen <= nseg << 18 picks the fused kernel, each corner's neighbours the three-kernel path; the
    results are the oracle's on both sides of every threshold"""
    c = D.auto_corner(nseg, mf, plus)
    W.set_option("reasm_path", 0)
    W.set_option("reasm_cfg", 0)
    try:
        for flags in (0, D.CTL):
            run(dev, c, mf, (0, 0), flags, D.oracle(c, mf, flags), "auto nseg %d max_frames %d buflen +%d flags %d"
                % (nseg, mf, plus, flags), buflen=c[4]["buflen"])
    finally:
        W.set_option("reasm_path", 0)


def test_forced_fused_above_64_frames_takes_the_three_kernel_path(dev):
    """reasm_path 1 with max_frames 65: the fused kernel's body table holds 64 frames, so the call
    runs the three-kernel path; a 65-frame segment is delivered whole"""
    c = case("frame_counts", (0, 0))
    orc = oracle("frame_counts", (0, 0), 65, 0)
    assert 65 in [int(x) for x in orc[1]["n_frames"]]
    W.set_option("reasm_path", 1)
    try:
        run(dev, c, 65, (0, 0), 0, orc, "forced fused, max_frames 65")
    finally:
        W.set_option("reasm_path", 0)
