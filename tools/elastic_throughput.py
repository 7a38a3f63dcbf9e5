#!/usr/bin/env python3
"""Cost of batched elastic tensors (SevenNetCalculator.elastic_many) against the same rule scripted on the host.

  workload   B rattled Si 2x2x2 cells (64 atoms, the cells of tools/neb_throughput.py before the vacancy is cut), clamped ions,
             nfree = 2: 13 copies per cell, SevenNet-0 shape
  (a)        elastic_many
  (b)        the same strained copies built on the host (tests/elastic_ref.py) and sent through compute_many in chunks of the same
             atom budget, the stresses and forces brought down and reduced to S, L and C with numpy

Device-synchronised wall clock after warm-up; the legs are interleaved ((a), (b), (a), (b), ...) in one process on one device,
median of --reps.  The report goes to stdout and to --out.

    python tools/elastic_throughput.py [--reps 5] [--B 24] [--budget 32768] [--out profiles/elastic_throughput.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from relax_throughput import _calc      # noqa: E402

DELTA, NFREE, N = 0.005, 2, 64


def make_cells(B):
    from sevennet_amd.neighbor import diamond_cubic
    return [(np.full(N, 14),) + diamond_cubic(5.431, (2, 2, 2), 0.05, seed) for seed in range(B)]


def host_elastic(calc, systems, budget):
    """(b): all copies through compute_many in chunks of at most `budget` atoms -> (S per system, engine calls)"""
    import elastic_ref
    copies = [(b, j, q) for b in range(len(systems)) for j in range(6) for q in elastic_ref.STENCIL[NFREE]] + [(b, 0, 0) for b in range(len(systems))]
    per = max(1, budget // N)
    res, calls = [], 0
    for c0 in range(0, len(copies), per):
        chunk = copies[c0:c0 + per]
        res += calc.compute_many([systems[b][0] for b, _, _ in chunk], [elastic_ref.strained(systems[b][1], j, q, DELTA) for b, j, q in chunk],
                                 np.stack([elastic_ref.strained(systems[b][2], j, q, DELTA) for b, j, q in chunk]), [True] * 3)
        calls += 1
    out = []
    for b in range(len(systems)):
        S, L = np.zeros((6, 6)), np.zeros((6, 3 * N))
        for j in range(6):
            pair = res[(6 * b + j) * NFREE:(6 * b + j + 1) * NFREE]
            S[:, j] = elastic_ref.difference([r['stress'] for r in pair], NFREE, DELTA)
            L[j] = elastic_ref.difference([r['forces'].reshape(-1) for r in pair], NFREE, DELTA)
        elastic_ref.moduli(elastic_ref.finish(S)[0])
        out.append(S)
    return out, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--B', type=int, default=24)
    ap.add_argument('--budget', type=int, default=32768)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'elastic_throughput.txt'))
    a = ap.parse_args()
    import torch
    from sevennet_amd.model_spec import sevennet_0_config
    B = a.B
    calc = _calc(sevennet_0_config(), [14])
    systems = make_cells(B)
    args = ([z for z, _, _ in systems], [p for _, p, _ in systems], np.stack([c for _, _, c in systems]), [True] * 3)
    legs = {'(a) elastic_many': lambda: calc.elastic_many(*args, delta=DELTA, nfree=NFREE, max_atoms_per_call=a.budget),
            '(b) host copies over chunked compute_many': lambda: host_elastic(calc, systems, a.budget)}
    for fn in legs.values():   # warm-up
        fn()
    times, last = {name: [] for name in legs}, {}
    for _ in range(a.reps):   # interleaved: each repetition runs every leg once
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    info = dict(calc.elastic_info)
    n_copies = B * (6 * NFREE + 1)
    lines = [f'elastic tensors: B = {B} rattled Si 2x2x2 cells ({N} atoms), clamped ions, nfree = {NFREE}, delta = {DELTA}: {n_copies} copies, '
             f'SevenNet-0 shape, random weights, at most {a.budget} atoms per call; legs interleaved, median (min .. max) of {a.reps} after warm-up']
    med = {}
    for name, ts in times.items():
        med[name] = float(np.median(ts))
        lines.append(f'  {name:<46} {med[name] * 1e3:10.2f} ms ({min(ts) * 1e3:.2f} .. {max(ts) * 1e3:.2f})')
    names = list(legs)
    dS = max(np.abs(r['stress_strain'] - s).max() for r, s in zip(last[names[0]], last[names[1]][0]))
    lines.append(f'  (a) makes {info["n_force_calls"]} engine calls, (b) {last[names[1]][1]}; elastic_many info {info}')
    lines.append(f'  (a) / (b) = {med[names[0]] / med[names[1]]:.3f}; largest |S difference| (a) against (b): {dS:.2e} eV/A^3')
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
