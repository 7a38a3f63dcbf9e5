#!/usr/bin/env python3
"""Cost of batched harmonic analysis (SevenNetCalculator.vibrations_many) against what a user had before it.

  workload   B vacancy cells (the rattled 2x2x2 Si cell with site 4 removed, 63 atoms: the bands' initial images of
             tools/neb_throughput.py), every atom displaced, nfree = 2: 379 copies per cell, SevenNet-0 shape
  (a)        vibrations_many
  (b)        the same copies built on the host and sent through compute_many in chunks of the same atom budget, the forces
             brought down and reduced to Hessians and spectra with numpy (tests/vib_ref.py)
  (c)        one compute call per copy, which is what ASE's Vibrations does: timed on --single-sample copies and scaled to
             all of them (the line says so)

Device-synchronised wall clock after warm-up; the legs are interleaved ((a), (b), (c), (a), (b), (c), ...) in one process on one
device, median of --reps.  The report goes to stdout and to --out.

    python tools/vib_throughput.py [--reps 3] [--B 24] [--budget 32768] [--single-sample 379] [--out profiles/vib_throughput.txt]
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

from neb_throughput import make_bands   # noqa: E402
from relax_throughput import _calc      # noqa: E402

DELTA, NFREE, MASS_SI = 0.01, 2, 28.0855


def host_copies(pos):
    """the 2 x 3 n displaced copies of one structure in the order of the rule (atom, axis, q = -1, +1)"""
    import vib_ref
    return [vib_ref.displaced(pos, a, i, q, DELTA) for a in range(len(pos)) for i in range(3) for q in vib_ref.STENCIL[NFREE]]


def host_vibrations(calc, systems, budget):
    """(b): all copies through compute_many in chunks of at most `budget` atoms -> (Hessians, engine calls)"""
    import vib_ref
    copies = [(b, p) for b, (z, pos, cell) in enumerate(systems) for p in host_copies(pos) + [pos]]
    per = max(1, budget // 63)
    forces, calls = [], 0
    for c0 in range(0, len(copies), per):
        chunk = copies[c0:c0 + per]
        res = calc.compute_many([systems[b][0] for b, _ in chunk], [p for _, p in chunk], np.stack([systems[b][2] for b, _ in chunk]), [True] * 3)
        forces += [r['forces'] for r in res]
        calls += 1
    out, j = [], 0
    for z, pos, cell in systems:
        n = len(pos)
        D = np.stack([vib_ref.row([forces[j + 2 * r].reshape(-1), forces[j + 2 * r + 1].reshape(-1)], NFREE, DELTA) for r in range(3 * n)])
        j += 2 * 3 * n + 1
        H, Hm, _ = vib_ref.finish(D, np.full(n, MASS_SI))
        vib_ref.spectrum(Hm)
        out.append(H)
    return out, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--B', type=int, default=24)
    ap.add_argument('--budget', type=int, default=32768)
    ap.add_argument('--single-sample', type=int, default=379)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vib_throughput.txt'))
    a = ap.parse_args()
    import torch
    from sevennet_amd.model_spec import sevennet_0_config
    B = a.B
    calc = _calc(sevennet_0_config(), [14])
    systems = [(z, im[0], cell) for z, im, cell in make_bands(B, 1)]
    args = ([z for z, _, _ in systems], [p for _, p, _ in systems], [np.full(63, MASS_SI)] * B, np.stack([c for _, _, c in systems]), [True] * 3)
    n_copies = B * (NFREE * 3 * 63 + 1)
    sample = [(systems[0][0], p, systems[0][2]) for p in (host_copies(systems[0][1]) + [systems[0][1]])[:a.single_sample]]
    legs = {'(a) vibrations_many': lambda: calc.vibrations_many(*args, delta=DELTA, nfree=NFREE, max_atoms_per_call=a.budget),
            '(b) host copies over chunked compute_many': lambda: host_vibrations(calc, systems, a.budget),
            f'(c) one compute per copy, {len(sample)} copies': lambda: [calc.compute(z, p, c, [True] * 3) for z, p, c in sample]}
    calc.vibrations_many(*[x[:2] for x in args[:4]], [True] * 3, delta=DELTA, nfree=NFREE, max_atoms_per_call=a.budget)   # warm-up on two cells
    host_vibrations(calc, systems[:1], a.budget)
    calc.compute(*sample[0], [True] * 3)
    times, last = {name: [] for name in legs}, {}
    for _ in range(a.reps):   # interleaved: each repetition runs every leg once
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    info = dict(calc.vib_info)
    lines = [f'harmonic analysis: B = {B} vacancy cells of the rattled Si 2x2x2 cell (63 atoms), all atoms, nfree = {NFREE}, delta = {DELTA} A: '
             f'{n_copies} copies, SevenNet-0 shape, random weights, at most {a.budget} atoms per call; legs interleaved, median (min .. max) '
             f'of {a.reps} after warm-up']
    med = {}
    for name, ts in times.items():
        med[name] = float(np.median(ts))
        lines.append(f'  {name:<46} {med[name] * 1e3:10.2f} ms ({min(ts) * 1e3:.2f} .. {max(ts) * 1e3:.2f})')
    names = list(legs)
    ta, tb = med[names[0]], med[names[1]]
    tc = med[names[2]] * n_copies / len(sample)
    dH = max(np.abs(r['hessian'] - h).max() for r, h in zip(last[names[0]], last[names[1]][0]))
    lines.append(f'  (c) scaled from {len(sample)} to all {n_copies} copies: {tc * 1e3:.2f} ms ({med[names[2]] * 1e3 / len(sample):.3f} ms per call)')
    lines.append(f'  (a) makes {info["n_force_calls"]} engine calls, (b) {last[names[1]][1]}; vibrations_many info {info}')
    lines.append(f'  (a) / (b) = {ta / tb:.3f}, (a) / (c) = {ta / tc:.4f}; largest |Hessian difference| (a) against (b): {dH:.2e} eV/A^2')
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
