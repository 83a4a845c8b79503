"""bench.py --dump-outputs: the dump's chunk sums and seeded byte sample against numpy (no GPU)."""
import numpy as np
import pytest

import bench

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("nbytes,sums_max", [(0, 1 << 20), (4096, 1 << 20), (3 * 4096 + 17, 1 << 20),
                                             (40 * 4096 + 5, 8)])
def test_dump_bytes_sums_every_byte(tmp_path, monkeypatch, nbytes, sums_max):
    """chunk sums cover every byte of the buffer (short last chunk included, chunk doubled until
    at most DUMP_SUMS_MAX sums), the sample holds the buffer's bytes, both of the stated dtypes"""
    monkeypatch.setattr(bench, "DUMP_SUMS_MAX", sums_max)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 1000)
    a = np.random.default_rng(nbytes).integers(0, 256, nbytes + 256, dtype=np.uint8)
    bench.dump_bytes(str(tmp_path), "wire", torch.from_numpy(a), nbytes, torch)
    sums = np.load(tmp_path / "wire_chunk_sums.npy")
    smp = np.load(tmp_path / "wire_sample.npy")
    assert sums.dtype == np.float64 and smp.dtype == np.float32
    assert len(sums) <= sums_max
    chunk = 4096
    while (nbytes + chunk - 1) // chunk > sums_max:
        chunk *= 2
    exp = [int(a[o:min(o + chunk, nbytes)].sum(dtype=np.int64)) for o in range(0, nbytes, chunk)]
    assert sums.tolist() == exp
    assert sums.sum() == a[:nbytes].sum(dtype=np.int64)
    assert len(smp) == min(nbytes, 1000)
    assert np.array_equal(smp, a[bench.dump_sample_positions(nbytes)].astype(np.float32))
    bench.dump_bytes(str(tmp_path), "again", torch.from_numpy(a), nbytes, torch)
    assert np.array_equal(np.load(tmp_path / "again_sample.npy"), smp)        # seeded positions
