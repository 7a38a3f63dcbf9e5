#!/usr/bin/env python3
"""Cost of the MD observables accumulated on the device (md_many(..., observe=Observe(...))) against what a user had before
them: md_many with traj_every = every, the frames copied to the host and post-processed in numpy.

  B rattled 2x2x2 Si cells (64 atoms), SevenNet-0 shape, random weights, NVE at 300 K, --steps steps, one sample every --every:
    (a) md_many                               no observables, no trajectory
    (b) md_many, observe=                     RDF (--rmax, --bins) and MSD / VACF (--lags, a new origin every sample)
    (c) md_many, traj_every = every           the frames come to the host; no velocities: a VACF cannot be formed from them
    (d) (c) + the numpy restatement           RDF and MSD of (b) from the frames of (c), tests/observe_ref.py on the host

Device-synchronised wall clock after warm-up; the legs are interleaved ((a), (b), (c), (d), (a), ...) in one process on one
device, median of --reps.  The report goes to stdout and to --out.  --only-observe runs (b) alone, for a kernel trace (per
sample one snet_obs_rdf and one snet_obs_correlate launch and two device-to-device copies).

    python tools/observe_throughput.py [--reps 5] [--B 24] [--steps 60] [--every 2] [--rmax 5.0] [--bins 100] [--lags 16]
                                       [--out profiles/observe_throughput.txt] [--only-observe]
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

MASS_SI = 28.0855


def host_observables(results, cells, rmax, bins, lags):
    """the restatement on the frames of a traj_every run -> per system (counts, msd_sum)"""
    import observe_ref as ref
    out = []
    for r, cell in zip(results, cells):
        traj = r['trajectory']
        n = traj.shape[1]
        kind = np.zeros(n, int)
        counts = sum(ref.rdf_counts(x, kind, 1, cell, [True] * 3, rmax, bins)[0] for x in traj)
        msd = ref.correlate(traj, np.zeros_like(traj), np.full(n, MASS_SI), kind, 1, lags, 1)[0]
        out.append((counts, msd))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--B', type=int, default=24)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--every', type=int, default=2)
    ap.add_argument('--rmax', type=float, default=5.0)
    ap.add_argument('--bins', type=int, default=100)
    ap.add_argument('--lags', type=int, default=16)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'observe_throughput.txt'))
    ap.add_argument('--only-observe', action='store_true')
    a = ap.parse_args()
    import torch
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.neighbor import diamond_cubic
    from sevennet_amd.observe import Observe
    B, K = a.B, a.steps
    calc = _calc(sevennet_0_config(), [14])
    cells = [diamond_cubic(5.431, (2, 2, 2), 0.05, seed) for seed in range(B)]
    args = ([np.full(64, 14)] * B, [p for p, _ in cells], [np.full(64, MASS_SI)] * B, np.stack([c for _, c in cells]), np.array([[True] * 3] * B))
    obs = Observe(every=a.every, rdf_rmax=a.rmax, rdf_bins=a.bins, lags=a.lags, origin_every=1)
    run = lambda **kw: calc.md_many(*args, 1.0, K, temperature=300.0, seed=1, **kw)   # noqa: E731
    run(observe=obs)   # warm-up
    if a.only_observe:
        run(observe=obs)
        print(f'md_many with observe: B = {B}, {K} steps, info {calc.md_info}')
        return
    legs = {'(a) md_many': lambda: run(),
            '(b) md_many, observe=': lambda: run(observe=obs),
            '(c) md_many, traj_every = every': lambda: run(traj_every=a.every),
            '(d) (c) + numpy restatement on the host': lambda: (lambda r: (r, host_observables(r, args[3], a.rmax, a.bins, a.lags)))(run(traj_every=a.every))}
    times, last = {name: [] for name in legs}, {}
    for _ in range(a.reps):   # interleaved: each repetition runs every leg once
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    n_samples = K // a.every + 1
    lines = [f'B = {B} rattled Si 2x2x2 cells (64 atoms), SevenNet-0 shape, random weights, NVE from 300 K, {K} steps of 1 fs, a sample '
             f'every {a.every} steps ({n_samples} samples); RDF to {a.rmax} A in {a.bins} bins, {a.lags} lags, every sample an origin; '
             f'one window of {K} steps per leg and repetition, legs interleaved, median (min .. max) of {a.reps} repetitions after warm-up']
    med = {}
    for name, ts in times.items():
        med[name] = float(np.median(ts))
        lines.append(f'  {name:<42} {med[name] * 1e3:9.2f} ms ({min(ts) * 1e3:.2f} .. {max(ts) * 1e3:.2f})  = {med[name] * 1e3 / K:7.3f} ms per step')
    ta, tb, tc, td = (med[k] for k in legs)
    lines.append(f'  (b) - (a) = {(tb - ta) * 1e3 / n_samples:.3f} ms per sample on the device; (d) - (a) = {(td - ta) * 1e3 / n_samples:.3f} ms per '
                 f'sample through the host ((c) - (a) = {(tc - ta) * 1e3 / n_samples:.3f} ms of it are the frames); (b) / (a) = {tb / ta:.3f}, '
                 f'(d) / (a) = {td / ta:.3f}')
    dev, (_, host) = last['(b) md_many, observe='], last['(d) (c) + numpy restatement on the host']
    same = all(np.array_equal(r['observables']['rdf']['counts'][0, 0], h[0][0, 0]) for r, h in zip(dev, host))
    n_or = dev[0]['observables']['n_origins']
    err = max(np.abs(r['observables']['msd'][0] - h[1][0] / (n_or * 64)).max() for r, h in zip(dev, host))
    lines.append(f'  (b) against (d): pair counts identical: {same}; largest |msd difference| {err:.2e} A^2 (the two runs move on the same bits)')
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
