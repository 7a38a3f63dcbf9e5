#!/usr/bin/env python3
"""Cost of batched constant-pressure MD (SevenNetCalculator.md_many with pressure=) against the fixed-cell loop it extends and
against what a user had before it: the same step rule on the host (tests/md_npt_ref.py) over compute_many, forces and stress
down and positions and cells up every step.

  per-step cost     B rattled 64-atom Si cells, SevenNet-0 shape, Langevin at 300 K, --steps steps:
                    (a) md_many with a pressure, (b) md_many at fixed cells, (c) the restatement on the host over
                    compute_many, system by system, (d) the bare compute_many calls of (c)

Device-synchronised wall clock after warm-up, median of --reps, all in one process.  --only-npt runs (a) alone, for a kernel
trace (one snet_mdb_npt_step launch per step).

    python tools/npt_throughput.py [--reps 5] [--B 216] [--steps 50] [--only-npt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from relax_throughput import _calc, _timed   # noqa: E402

DT, T, FRICTION, SEED = 1.0, 300.0, 0.01, 0
NPT = dict(pressure=0.0, compressibility=60.0, barostat_time=1000.0)
MASS_SI = 28.0855


def host_npt(calc, nums, poss, masses, cells, pbcs, vels, steps):
    """the restatement's NPT step on the host, one compute_many call per launch for all systems: -> (states, engine calls)"""
    import md_npt_ref as ref
    import md_ref
    c1, c2 = md_ref.langevin_coefficients(FRICTION, DT)
    kT, bt = md_ref.KB * T, NPT['compressibility'] / NPT['barostat_time']
    states = [ref.npt_init(p, c, v) for p, c, v in zip(poss, cells, vels)]
    for k in range(steps + 1):
        res = calc.compute_many(nums, [s['pos'] for s in states], np.stack([s['cell'] for s in states]), pbcs)
        phase = (md_ref.FINISH if k > 0 else 0) | (md_ref.START if k < steps else 0)
        states = [ref.npt_step(s, r['forces'], -r['stress'][[0, 1, 2, 5, 3, 4]] * abs(np.linalg.det(s['cell'])), m, kT, NPT['pressure'],
                               bt, DT, c1, c2, SEED, b, phase, 0.1, calc.cutoff / 64)[0]
                  for b, (s, r, m) in enumerate(zip(states, res, masses))]
    return states, steps + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--B', type=int, default=216)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--only-npt', action='store_true')
    a = ap.parse_args()
    import md_ref
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.neighbor import diamond_cubic
    B, K = a.B, a.steps
    pbcs = np.array([[True] * 3] * B)
    calc = _calc(sevennet_0_config(), [14])
    built = [diamond_cubic(5.431, (2, 2, 2), 0.05, seed) for seed in range(B)]
    nums, poss, cs = [np.full(64, 14)] * B, [p for p, _ in built], np.stack([c for _, c in built])
    masses = [np.full(64, MASS_SI)] * B
    vels = [md_ref.init_velocities(m, md_ref.KB * T, seed=100 + b, sys_id=b) for b, m in enumerate(masses)]
    kw = dict(velocities=vels, temperature=T, friction=FRICTION, seed=SEED, log_every=10)
    npt = lambda: calc.md_many(nums, poss, masses, cs, pbcs, DT, K, **kw, **NPT)   # noqa: E731
    npt()   # warm-up
    if a.only_npt:
        npt()
        print(f'md_many with a pressure: B = {B}, {K} steps, info {calc.md_info}')
        return
    print(f'per-step cost: B = {B} rattled Si 2x2x2 cells (64 atoms), SevenNet-0 shape, random weights, Langevin at {T} K, {K} steps; '
          f'median (min .. max) of {a.reps} after warm-up')
    fixed = lambda: calc.md_many(nums, poss, masses, cs, pbcs, DT, K, **kw)   # noqa: E731
    fixed()
    host_npt(calc, nums, poss, masses, cs, pbcs, vels, 2)
    t_a = _timed(npt, a.reps)
    info = dict(calc.md_info)
    t_b = _timed(fixed, a.reps)
    t_c = _timed(lambda: host_npt(calc, nums, poss, masses, cs, pbcs, vels, K), a.reps)
    t_d = _timed(lambda: [calc.compute_many(nums, poss, cs, pbcs) for _ in range(K + 1)], a.reps)
    for name, t in (('(a) md_many, pressure given', t_a), ('(b) md_many, fixed cells', t_b),
                    ('(c) host restatement over compute_many', t_c), (f'(d) {K + 1} bare compute_many calls', t_d)):
        print(f'  {name:<42} {t[0] * 1e3:9.2f} ms ({t[1] * 1e3:.2f} .. {t[2] * 1e3:.2f})  = {t[0] * 1e3 / (K + 1):6.3f} ms per engine call')
    dcell = max(np.abs(r['cell'] - s['cell']).max() for r, s in zip(t_a[3], t_c[3][0]))
    failed = sum(r['status'] != 'ok' for r in t_a[3])
    print(f'  all four make {K + 1} engine calls; md_many info {info}; (a) - (b) = {(t_a[0] - t_b[0]) * 1e3 / K:.3f} ms per step, '
          f'(a) / (c) = {t_a[0] / t_c[0]:.3f}')
    print(f'  largest |cell difference| after {K} steps, (a) against (c): {dcell:.2e} A; systems refused by the guard: {failed}')


if __name__ == '__main__':
    main()
