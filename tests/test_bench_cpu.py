"""CPU: bench.py's --dump-outputs writer keeps the outputs under its size bound with a sample that is the same on every run."""
import os

import numpy as np

import bench


def test_dump_outputs_bound_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 40_000)
    rng = np.random.default_rng(5)
    arrays = {'energy': np.array([-1.25]), 'virial': rng.normal(size=6), 'forces': rng.normal(size=(1000, 3)).astype(np.float32),
              'dE_dr': rng.normal(size=(5000, 3)).astype(np.float32)}
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), dict(arrays))
    got = {f[:-4]: np.load(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')}
    assert set(got) == set(arrays)
    assert sum(v.nbytes for v in got.values()) <= 40_000
    # what fits stays whole; the largest array is cut to rows of itself, in order, the same rows in both runs
    for k in ('energy', 'virial', 'forces'):
        assert got[k].dtype == arrays[k].dtype and np.array_equal(got[k], arrays[k])
    d = got['dE_dr']
    assert d.dtype == np.float32 and 0 < len(d) < 5000
    rows = [int(np.flatnonzero((arrays['dE_dr'] == r).all(1))[0]) for r in d]
    assert rows == sorted(rows)
    assert np.array_equal(d, np.load(tmp_path / 'b' / 'dE_dr.npy'))


def test_dump_outputs_whole_when_it_fits(tmp_path):
    arrays = {'energy': np.array([3.0]), 'forces': np.ones((97336, 3), np.float32), 'dE_dr': np.ones((2725408, 3), np.float32)}
    bench.dump_outputs(str(tmp_path), dict(arrays))
    for k, v in arrays.items():
        assert np.array_equal(np.load(tmp_path / f'{k}.npy'), v)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) < 64_000_000
