"""bench.py's --dump-outputs writer (dump_outputs) on CPU tensors: the sampled form a full-size output takes."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_samples_large_outputs_reproducibly(tmp_path):
    n, d, world, rank, lo = 5000, 128, 1024, 3, 7 * 5000    # world 1024: the row budget per rank is 64 rows of 512 B
    out = torch.rand(n, d, generator=torch.Generator().manual_seed(0))
    for sub in ("a", "b"):
        bench.dump_outputs(torch, out, str(tmp_path / sub), rank, world, lo=lo)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["rank3_scatter_add_col_sums.npy", "rank3_scatter_add_row_ids.npy", "rank3_scatter_add_rows.npy"]
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    ids = np.load(tmp_path / "a" / names[1])
    rows = np.load(tmp_path / "a" / names[2])
    k = bench.DUMP_ROW_BYTES // world // (d * 4)
    assert ids.shape == (k,) and rows.shape == (k, d)
    assert np.all(np.diff(ids) > 0) and ids[0] >= lo and ids[-1] < lo + n
    assert np.array_equal(rows, out.numpy()[ids.astype(np.int64) - lo])
    assert np.allclose(np.load(tmp_path / "a" / names[0]), out.double().sum(0).numpy(), rtol=1e-12, atol=0)
