#!/usr/bin/env python3
"""Throughput of batched D3: B rattled 64-atom Si cells at the default cutoffs (9000 / 1600 bohr^2, damp_bj, pbe) as a loop
over `compute` and as ONE `compute_many` call, for D3Calculator and for SevenNetD3Calculator (SevenNet-0 shape, seeded random
weights).  Device-synchronised wall clock after warm-up, median of --reps.

    python tools/d3_batch_throughput.py [--reps 5] [--sizes 1,16,64,216]
    python tools/d3_batch_throughput.py --many-only 216     # one warm-up and one compute_many of D3Calculator (kernel trace)
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
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def _cells(B):
    from sevennet_amd.neighbor import diamond_cubic
    cells = [diamond_cubic(5.431, (2, 2, 2), 0.05, seed) for seed in range(B)]
    return ([np.full(64, 14) for _ in cells], [p for p, _ in cells], np.stack([c for _, c in cells]), np.array([[True] * 3] * B))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='1,16,64,216')
    ap.add_argument('--many-only', type=int, default=0, help='only D3Calculator.compute_many of this many cells, twice')
    a = ap.parse_args()
    from sevennet_amd.d3 import D3Calculator, SevenNetD3Calculator
    d3 = D3Calculator()
    if a.many_only:
        args = _cells(a.many_only)
        for _ in range(2):   # warm-up, then the traced call
            d3.compute_many(*args)
        print(f'D3Calculator.compute_many: 2 calls of B = {a.many_only}')
        return
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.synthetic import random_state_dict
    cfg = sevennet_0_config()
    cfg['_type_map'] = {14: 0}
    sd3 = SevenNetD3Calculator((cfg, random_state_dict(cfg, 0)), file_type='model_instance', device='cuda:0')
    sizes = [int(s) for s in a.sizes.split(',')]
    print(f'D3 damp_bj / pbe, cutoffs 9000 / 1600 bohr^2; rattled Si 2x2x2 cells (64 atoms); SevenNetD3Calculator: SevenNet-0 '
          f'shape, random weights; median of {a.reps} after warm-up')
    print(f'{"":<22} {"B":>4} | {"loop":>10} {"str/s":>8} | {"compute_many":>12} {"str/s":>8} | {"speed-up":>8}')
    rows = {}
    for name, calc in (('D3Calculator', d3), ('SevenNetD3Calculator', sd3)):
        for B in sizes:
            nums, poss, cs, pbcs = _cells(B)

            def loop():
                return [calc.compute(n, p, c, pb) for n, p, c, pb in zip(nums, poss, cs, pbcs)]

            def many():
                return calc.compute_many(nums, poss, cs, pbcs)

            loop()
            many()   # warm-up
            t_loop, t_many = _timed(loop, a.reps), _timed(many, a.reps)
            rows[name, B] = (t_loop, t_many)
            print(f'{name:<22} {B:>4} | {t_loop * 1e3:>8.2f}ms {B / t_loop:>8.0f} | {t_many * 1e3:>10.2f}ms {B / t_many:>8.0f} | '
                  f'{t_loop / t_many:>7.1f}x', flush=True)
    if ('D3Calculator', 216) in rows:
        d_loop, d_many = rows['D3Calculator', 216]
        s_loop, s_many = rows['SevenNetD3Calculator', 216]
        print(f'B = 216: D3Calculator compute_many / compute loop = {d_loop / d_many:.1f}x structures/s (expected >= 3x); '
              f'SevenNetD3Calculator {s_loop / s_many:.1f}x; D3 share of a SevenNetD3Calculator call: loop '
              f'{d_loop / s_loop:.0%}, compute_many {d_many / s_many:.0%}')


if __name__ == '__main__':
    main()
