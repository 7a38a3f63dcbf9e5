#!/usr/bin/env python3
"""Throughput of batched evaluation: B rattled 64-atom Si cells (SevenNet-0 shape, seeded random weights) as a loop over
SevenNetCalculator.compute, as ONE compute_many call, and -- for the atom and edge count of B = 216 -- one 12x12x12
supercell (13 824 atoms) through compute.  Device-synchronised wall clock after warm-up, median of --reps; graph build
and model time are shown separately (the graph build includes the pair numbering, the model the readbacks of compute).

    python tools/batch_throughput.py [--reps 5] [--sizes 1,16,64,216]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps):
    import torch
    ts, r = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='1,16,64,216')
    a = ap.parse_args()
    import torch
    from sevennet_amd.batch import build_batch_graph
    from sevennet_amd.calculator import SevenNetCalculator
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.neighbor import diamond_cubic
    from sevennet_amd.neighbor_gpu import build_graph_gpu
    from sevennet_amd.synthetic import random_state_dict
    cfg = sevennet_0_config()
    cfg['_type_map'] = {14: 0}
    calc = SevenNetCalculator((cfg, random_state_dict(cfg, 0)), file_type='model_instance', device='cuda:0')
    eng, rc, dev = calc.model, calc.cutoff, 'cuda:0'
    sizes = [int(s) for s in a.sizes.split(',')]
    cells = [diamond_cubic(5.431, (2, 2, 2), 0.05, seed) for seed in range(max(sizes))]
    pbc = [True] * 3
    print(f'SevenNet-0 shape, random weights, rattled Si 2x2x2 cells (64 atoms), cutoff {rc} A; median of {a.reps} after warm-up')
    print(f'{"B":>4} {"atoms":>6} {"edges":>8} | {"loop: total":>11} {"build":>8} {"model":>8} {"str/s":>8} | '
          f'{"batch: total":>12} {"build":>8} {"model":>8} {"str/s":>8} | {"speed-up":>8}')
    rows = {}
    for B in sizes:
        sys_ = cells[:B]
        nums = [np.full(64, 14) for _ in sys_]
        poss = [p for p, _ in sys_]
        cs = np.stack([c for _, c in sys_])
        pbcs = np.array([pbc] * B)
        types = [np.zeros(64, np.int64) for _ in sys_]

        def loop():
            return [calc.compute(n, p, c, pbc) for n, p, c in zip(nums, poss, cs)]

        def loop_build():
            return [build_graph_gpu(t, p, c, rc, device=dev, pbc=pbc) for t, p, c in zip(types, poss, cs)]

        def batch_build():
            return build_batch_graph(types, poss, cs, pbcs, rc, eng.spec.num_species, device=dev)

        for f in (loop, batch_build):
            f()   # warm-up
        t_loop, res = _timed(loop, a.reps)
        t_lb, gs = _timed(loop_build, a.reps)
        t_lm, _ = _timed(lambda: [eng.compute(g) for g in gs], a.reps)
        t_many, _ = _timed(lambda: calc.compute_many(nums, poss, cs, pbcs), a.reps)
        t_bb, gb = _timed(batch_build, a.reps)
        t_bm, _ = _timed(lambda: eng.compute(gb), a.reps)
        rows[B] = (t_loop, t_many, t_bm, gb.n_edges)
        print(f'{B:>4} {64 * B:>6} {gb.n_edges:>8} | {t_loop * 1e3:>9.2f}ms {t_lb * 1e3:>6.2f}ms {t_lm * 1e3:>6.2f}ms '
              f'{B / t_loop:>8.0f} | {t_many * 1e3:>10.2f}ms {t_bb * 1e3:>6.2f}ms {t_bm * 1e3:>6.2f}ms {B / t_many:>8.0f} | '
              f'{t_loop / t_many:>7.1f}x', flush=True)
    pos, cell = diamond_cubic(5.431, (12, 12, 12), 0.05, 0)
    n = np.full(len(pos), 14)
    calc.compute(n, pos, cell, pbc)
    t_sc, res = _timed(lambda: calc.compute(n, pos, cell, pbc), a.reps)
    t_sb, g = _timed(lambda: build_graph_gpu(np.zeros(len(pos), np.int64), pos, cell, rc, device=dev, pbc=pbc), a.reps)
    t_sm, _ = _timed(lambda: eng.compute(g), a.reps)
    print(f'supercell 12x12x12: {len(pos)} atoms, {res["num_edges"]} edges | compute total {t_sc * 1e3:.2f} ms, '
          f'build {t_sb * 1e3:.2f} ms, model {t_sm * 1e3:.2f} ms', flush=True)
    if 216 in rows:
        t_loop, t_many, t_bm, e = rows[216]
        print(f'B = 216: compute_many / compute loop = {t_loop / t_many:.1f}x structures/s (expected >= 10x); batch model time / '
              f'supercell model time = {t_bm / t_sm:.2f} (expected <= 1.25); batch edges {e} vs supercell {res["num_edges"]}')


if __name__ == '__main__':
    main()
