#!/usr/bin/env python3
"""Step rate of the batched drivers with the D3 term on the host against the D3 term on the device: SevenNetD3Calculator
(SevenNet-0 shape, seeded random weights; D3 damp_bj / pbe at the default cutoffs 9000 / 1600 bohr^2) on B rattled 8-atom Si
cells -- `relax_many` (a fixed number of FIRE steps: fmax 0, no repack) and `md_many` (NVE) with d3_term='host' and
d3_term='device', the two interleaved in one process.  Device-synchronised wall clock after one warm-up of each, median of
--reps; the per-step figure divides by the force calls of the run.  Writes profiles/d3_term_throughput.txt.

    python tools/d3_term_throughput.py [--reps 5] [--sizes 16,64,216] [--steps 20] [--out profiles/d3_term_throughput.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cells(B):
    from sevennet_amd.neighbor import diamond_cubic
    cells = [diamond_cubic(5.431, (1, 1, 1), 0.05, seed) for seed in range(B)]
    return ([np.full(8, 14) for _ in cells], [p for p, _ in cells], np.stack([c for _, c in cells]), np.array([[True] * 3] * B))


def _interleaved(fns, reps):
    """median wall clock of each callable, run in turn `reps` times"""
    import torch
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='16,64,216')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'd3_term_throughput.txt'))
    a = ap.parse_args()
    import torch
    from sevennet_amd.d3 import SevenNetD3Calculator
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.synthetic import random_state_dict
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    cfg = sevennet_0_config()
    cfg['_type_map'] = {14: 0}
    calc = SevenNetD3Calculator((cfg, random_state_dict(cfg, 0)), file_type='model_instance', device='cuda:0')
    lines = [f'D3 term of the batched drivers, host against device: SevenNetD3Calculator (SevenNet-0 shape, random weights; D3 damp_bj / '
             f'pbe, cutoffs 9000 / 1600 bohr^2) on B rattled Si cells of 8 atoms; {a.steps} steps per run; interleaved, median of '
             f'{a.reps} after warm-up; ms per force call (model + D3 + step kernel)',
             f'{"driver":<12} {"B":>4} | {"host":>9} {"device":>9} | {"host / device":>13} | same positions']
    print('\n'.join(lines), flush=True)
    for B in [int(s) for s in a.sizes.split(',')]:
        nums, poss, cs, pbcs = _cells(B)
        masses = [np.full(8, 28.0855)] * B
        runs = {
            'relax_many': lambda term: calc.relax_many(nums, poss, cs, pbcs, fmax=0.0, steps=a.steps, repack_below=0.0, d3_term=term),
            'md_many': lambda term: calc.md_many(nums, poss, masses, cs, pbcs, 1.0, a.steps, temperature=300.0, d3_term=term),
        }
        for name, run in runs.items():
            host, dev = run('host'), run('device')   # warm-up, and the check that the two do the same thing
            same = all(np.array_equal(h['positions'], d['positions']) for h, d in zip(host, dev))
            calls = (calc.relax_info if name == 'relax_many' else calc.md_info)['n_force_calls']
            t_host, t_dev = _interleaved([lambda: run('host'), lambda: run('device')], a.reps)
            lines.append(f'{name:<12} {B:>4} | {t_host / calls * 1e3:>7.2f}ms {t_dev / calls * 1e3:>7.2f}ms | {t_host / t_dev:>12.2f}x | {same}')
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
