#!/usr/bin/env python3
"""Cost of batched nudged elastic band (SevenNetCalculator.neb_many) against what a user had before it: the same rule on the
host (tests/neb_ref.py: improved tangent, springs, one FIRE per band from tests/relax_ref.py) over compute_many, every image's
forces and energy down and the positions up every step.

  per-step cost     B bands of a vacancy hop in the rattled 2x2x2 Si cell (63 atoms), --images moving images each, SevenNet-0
                    shape, fmax = 0 (nothing converges), --steps steps:
                    (a) neb_many, (b) the restatement on the host over one compute_many call per step for the moving images
                    of all bands, (c) the bare compute_many calls of (b)

Device-synchronised wall clock after warm-up; the three legs are interleaved ((a), (b), (c), (a), (b), (c), ...) in one process
on one device, median of --reps.  The report goes to stdout and to --out.  --only-neb runs (a) alone, for a kernel trace (one
snet_neb_forces and one snet_fire_step launch per step).

    python tools/neb_throughput.py [--reps 5] [--B 24] [--images 5] [--steps 30] [--out profiles/neb_throughput.txt] [--only-neb]
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

from relax_throughput import _calc   # noqa: E402

K_SPRING = 0.1


def make_bands(B, m):
    """B x (numbers [63], images [m + 2, 63, 3], cell): site 4 of the rattled 64-atom cell is removed and site 0 moves into it"""
    from sevennet_amd.neb import interpolate_band
    from sevennet_amd.neighbor import diamond_cubic
    out = []
    for seed in range(B):
        pos, cell = diamond_cubic(5.431, (2, 2, 2), 0.05, seed)
        keep = np.arange(len(pos)) != 4
        initial, final = pos[keep].copy(), pos[keep].copy()
        final[0] = pos[4]
        out.append((np.full(63, 14), interpolate_band(initial, final, m + 2, cell, [True] * 3), cell))
    return out


def host_neb(calc, bands, steps):
    """the restatement's band step on the host: the endpoints once, then per step ONE compute_many call for the moving images of
    all bands, and one more for all images at the final positions (what neb_many returns) -> (final images per band, engine calls)"""
    import neb_ref
    import relax_ref
    pbc = [True] * 3
    nums = [z for z, im, _ in bands for _ in im[1:-1]]
    cells = np.stack([c for _, im, c in bands for _ in im[1:-1]])
    ends = calc.compute_many([z for z, _, _ in bands for _ in range(2)], [im[j] for _, im, _ in bands for j in (0, -1)],
                             np.stack([c for _, _, c in bands for _ in range(2)]), pbc)
    states = [relax_ref.fire_init(im[1:-1].reshape(-1, 3)) for _, im, _ in bands]
    for _ in range(steps):
        res = iter(calc.compute_many(nums, [p for s, (_, im, _) in zip(states, bands) for p in s['pos'].reshape(im[1:-1].shape)], cells, pbc))
        for b, (_, im, cell) in enumerate(bands):
            m = len(im) - 2
            mine = [next(res) for _ in range(m)]
            cur = np.concatenate([im[:1], states[b]['pos'].reshape(m, -1, 3), im[-1:]])
            energies = [ends[2 * b]['energy']] + [r['energy'] for r in mine] + [ends[2 * b + 1]['energy']]
            f_neb, _, _ = neb_ref.neb_forces(cur, np.stack([r['forces'] for r in mine]), energies, cell, pbc, K_SPRING)
            states[b] = relax_ref.fire_step(states[b], f_neb.reshape(-1, 3), 0.0)[0]
    final = [np.concatenate([im[:1], s['pos'].reshape(len(im) - 2, -1, 3), im[-1:]]) for s, (_, im, _) in zip(states, bands)]
    calc.compute_many([z for z, im, _ in bands for _ in im], [p for f in final for p in f], np.stack([c for _, im, c in bands for _ in im]), pbc)
    return final, steps + 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--B', type=int, default=24)
    ap.add_argument('--images', type=int, default=5)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'neb_throughput.txt'))
    ap.add_argument('--only-neb', action='store_true')
    a = ap.parse_args()
    import torch
    from sevennet_amd.model_spec import sevennet_0_config
    B, K, m = a.B, a.steps, a.images
    calc = _calc(sevennet_0_config(), [14])
    bands = make_bands(B, m)
    args = ([z for z, _, _ in bands], [im for _, im, _ in bands], np.stack([c for _, _, c in bands]), [True] * 3)
    neb = lambda: calc.neb_many(*args, fmax=0.0, steps=K, k=K_SPRING)   # noqa: E731
    neb()   # warm-up
    if a.only_neb:
        neb()
        print(f'neb_many: B = {B} bands of {m} moving images, {K} steps, info {calc.neb_info}')
        return
    nums = [z for z, im, _ in bands for _ in im[1:-1]]
    moving = [p for _, im, _ in bands for p in im[1:-1]]
    cells = np.stack([c for _, im, c in bands for _ in im[1:-1]])
    legs = {'(a) neb_many': neb, '(b) host restatement over compute_many': lambda: host_neb(calc, bands, K),
            f'(c) {K} bare compute_many calls of (b)': lambda: [calc.compute_many(nums, moving, cells, [True] * 3) for _ in range(K)]}
    host_neb(calc, bands, 2)
    times, last = {name: [] for name in legs}, {}
    for _ in range(a.reps):   # interleaved: each repetition runs every leg once
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    info = dict(calc.neb_info)
    lines = [f'per-step cost: B = {B} bands of a vacancy hop in the rattled Si 2x2x2 cell (63 atoms), {m} moving images each, SevenNet-0 '
             f'shape, random weights, fmax = 0, {K} steps; legs interleaved, median (min .. max) of {a.reps} after warm-up']
    med = {}
    for name, ts in times.items():
        med[name] = float(np.median(ts))
        lines.append(f'  {name:<44} {med[name] * 1e3:9.2f} ms ({min(ts) * 1e3:.2f} .. {max(ts) * 1e3:.2f})  = {med[name] * 1e3 / K:7.3f} ms per step')
    ta, tb = med['(a) neb_many'], med['(b) host restatement over compute_many']
    got = [np.stack([im['positions'] for im in r['images']]) for r in last['(a) neb_many']]
    dpos = max(np.abs(g - h).max() for g, h in zip(got, last['(b) host restatement over compute_many'][0]))
    lines.append(f'  (a) and (b) make {K + 2} engine calls each (the endpoints, {K} steps, all images at the final positions); neb_many info {info}')
    lines.append(f'  (b) - (a) = {(tb - ta) * 1e3 / K:.3f} ms per step, (a) / (b) = {ta / tb:.3f}; largest |position difference| after {K} steps, '
                 f'(a) against (b): {dpos:.2e} A')
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
