"""bench.py --dump-outputs: the arrays as they land on disk.  CPU only (the benchmark itself runs on the GPU)."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_writes_float_arrays_and_the_same_sample_of_a_large_one(tmp_path):
    n = bench.DUMP_MAX_ELEMS + 1000
    arrays = {'metrics': [1.5, 0.25], 'weights': torch.arange(n, dtype=torch.float32),
              'half': torch.ones(3, dtype=torch.bfloat16), 'counter': torch.tensor([7])}
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {f[:-4]: np.load(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')}
    assert sorted(got) == sorted(arrays)
    assert got['metrics'].dtype == np.float64 and got['metrics'].tolist() == [1.5, 0.25]
    assert got['counter'].dtype == np.float64 and got['counter'].tolist() == [7.0]
    assert got['half'].dtype == np.float32 and got['half'].tolist() == [1.0] * 3
    w = got['weights']
    assert w.dtype == np.float32 and w.shape == (bench.DUMP_MAX_ELEMS,)
    assert (np.diff(w) > 0).all() and w[0] >= 0 and w[-1] < n            # distinct elements of the array, in order
    assert np.array_equal(w, np.load(tmp_path / 'b' / 'weights.npy'))     # the same sample on every run
