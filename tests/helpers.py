"""Shared test helpers: golden fixtures, oracle construction, layout conversion."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_ts_golden(name, parallel=False):
    d = np.load(os.path.join(GOLDEN, f'ts_oracle_{name}.npz'))
    cfg = json.loads(str(d['__pconfig__' if parallel else '__config__']))
    pre = 'pw::' if parallel else 'w::'
    sd = {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}
    return d, cfg, sd


def oracle_model(cfg, sd, dtype=torch.float64):
    from oracle.model import OracleModel
    return OracleModel(cfg, sd, dtype=dtype)


def irmul_to_mulir(x, irreps):
    """engine (ir_mul) rows -> reference (mul_ir) rows; irreps = sevennet_amd Irreps."""
    from sevennet_amd.irreps import irmul_to_mulir_index
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x[:, irmul_to_mulir_index(irreps)]


def synthetic_system(n_rep=(2, 2, 2), a=5.431, sigma=0.05, seed=0, cutoff=5.0, n_species=1):
    from sevennet_amd.neighbor import diamond_cubic, neighbor_list
    pos, cell = diamond_cubic(a, n_rep, sigma, seed)
    ei, ev, _ = neighbor_list(pos, cell, [True] * 3, cutoff)
    rng = np.random.default_rng(seed + 1)
    types = rng.integers(0, n_species, len(pos)) if n_species > 1 else np.zeros(len(pos), np.int64)
    return types, pos, cell, ei, ev


def three_small_systems(seed=0):
    """B = 3 systems of 2, 5 and 8 atoms as (species indices in {0, 1}, positions, cell, pbc): a periodic cell of 6 A, a molecule
    with a zero cell, a slab with pbc (T, T, F) -- the smallest sizes at which the segment arithmetic, a subset of the systems
    and the molecule box can each still go wrong"""
    from sevennet_amd.neighbor import diamond_cubic
    rng = np.random.default_rng(seed)
    mol = np.array([[0.0, 0.0, 0.0], [1.1, 0.0, 0.0], [-0.4, 1.0, 0.0], [0.2, -0.5, 1.0], [2.3, 0.4, -0.6]])
    slab, cell = diamond_cubic(5.431, (1, 1, 1), 0.08, seed)
    return [(np.array([0, 1]), np.array([[0.5, 0.4, 0.3], [2.1, 1.0, 0.7]]) + rng.normal(0, 0.05, (2, 3)), np.eye(3) * 6.0, [True] * 3),
            (np.array([0, 1, 1, 0, 1]), mol + rng.normal(0, 0.05, (5, 3)), np.zeros((3, 3)), [False] * 3),
            (rng.integers(0, 2, 8), slab, cell, [True, True, False])]


def packed_tiles_expected(row_ptr, lo, hi, group=8):
    """restatement of snet_edge_tiles_packed: greedy windows of <= 16 consecutive edges over <= 2 rows, per group of rows"""
    rp = [int(v) for v in row_ptr]
    e0, nodes = [], []
    for a in range(lo, hi, group):
        b = min(a + group, hi)
        e, n0 = rp[a], a
        while e < rp[b]:
            while rp[n0 + 1] <= e:
                n0 += 1
            n1 = n0 + 1
            while n1 < b and rp[n1 + 1] == rp[n1]:
                n1 += 1
            lim = rp[n1 + 1] if n1 < b else rp[n0 + 1]
            end = min(e + 16, lim)
            e0.append(e)
            nodes += [n0, n1 if end > rp[n0 + 1] else n0]
            e = end
    return e0 + [rp[hi]], nodes
