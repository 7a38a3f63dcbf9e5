#!/usr/bin/env python3
"""Cost of batched FIRE relaxation (SevenNetCalculator.relax_many) against what a user had before it: the same FIRE rule on
the host (tests/relax_ref.py) over compute_many, forces down and positions up every step.

  per-step cost     B rattled 64-atom Si cells, SevenNet-0 shape, fmax = 0 (nothing converges), --steps steps:
                    (a) relax_many, (b) host FIRE over compute_many (the restatement, system by system), (b') the same
                    rule vectorised over the batch in numpy, (c) the bare compute_many calls of (b)
  staggered         the mini model at fmax = 0.02 on cells rattled with sigma in [0.02, 0.15], two species: systems finish
                    at different steps; relax_many with repack_below 0 and 0.5 against the host loop, which evaluates every
                    system until the slowest is done

Device-synchronised wall clock after warm-up, median of --reps, all in one process.  --only-relax runs (a) alone, for a
kernel trace (one snet_fire_step launch per step).

    python tools/relax_throughput.py [--reps 5] [--B 216] [--steps 50] [--only-relax]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _timed(fn, reps):
    import torch
    ts, r = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts)), r


def host_fire(calc, nums, poss, cells, pbcs, fmax, steps):
    """the restatement's FIRE on the host, one compute_many call per step for all systems until the slowest is done, and one
    more at the final positions (what relax_many returns): -> (results, states, engine calls)"""
    import relax_ref
    states = [relax_ref.fire_init(p) for p in poss]
    calls = 0
    for _ in range(steps):
        res = calc.compute_many(nums, [s['pos'] for s in states], cells, pbcs)
        calls += 1
        states = [relax_ref.fire_step(s, r['forces'], fmax)[0] for s, r in zip(states, res)]
        if not any(s['active'] for s in states):
            break
    return calc.compute_many(nums, [s['pos'] for s in states], cells, pbcs), states, calls + 1


def host_fire_vectorised(calc, nums, poss, cells, pbcs, fmax, steps):
    """`host_fire` for systems of one size with the FIRE rule vectorised over the batch in numpy ([B,n,3] arrays): the host
    cost is then the readback, the dict building and the upload, not a Python loop over systems"""
    import relax_ref
    p = relax_ref.FIRE
    pos = np.stack(poss).astype(np.float64)
    B = len(pos)
    vel, dt, alpha = np.zeros_like(pos), np.full(B, p['dt_start']), np.full(B, p['alpha_start'])
    n_pos, active = np.zeros(B, np.int64), np.ones(B, bool)
    calls = 0
    for _ in range(steps):
        res = calc.compute_many(nums, list(pos), cells, pbcs)
        calls += 1
        f = np.stack([r['forces'] for r in res])
        active &= ~(np.sqrt((f * f).sum(2).max(1)) < fmax)
        if not active.any():
            break
        P = (f * vel).sum((1, 2))
        nf, nv = np.sqrt((f * f).sum((1, 2))), np.sqrt((vel * vel).sum((1, 2)))
        down = P > 0
        mixed = (1 - alpha)[:, None, None] * vel + (alpha / np.where(nf > 0, nf, 1.0) * nv)[:, None, None] * f
        grow = down & (n_pos > p['n_min'])
        dt_new = np.where(grow, np.minimum(dt * p['f_inc'], p['dt_max']), np.where(down, dt, dt * p['f_dec']))
        alpha_new = np.where(grow, alpha * p['f_alpha'], np.where(down, alpha, p['alpha_start']))
        v = np.where(down[:, None, None], mixed, 0.0) + dt_new[:, None, None] * f
        dr = dt_new[:, None, None] * v
        n = np.sqrt((dr * dr).sum((1, 2)))
        dr *= np.where(n > p['max_step'], p['max_step'] / np.where(n > 0, n, 1.0), 1.0)[:, None, None]
        m = active[:, None, None]
        pos, vel = np.where(m, pos + dr, pos), np.where(m, v, vel)
        dt, alpha = np.where(active, dt_new, dt), np.where(active, alpha_new, alpha)
        n_pos = np.where(active, np.where(down, n_pos + 1, 0), n_pos)
    return calc.compute_many(nums, list(pos), cells, pbcs), pos, calls + 1


def _calc(cfg, z):
    from sevennet_amd.calculator import SevenNetCalculator
    from sevennet_amd.synthetic import random_state_dict
    cfg = dict(cfg, _type_map={zz: k for k, zz in enumerate(z)})
    return SevenNetCalculator((cfg, random_state_dict(cfg, 0)), file_type='model_instance', device='cuda:0')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--B', type=int, default=216)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--only-relax', action='store_true')
    a = ap.parse_args()
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.neighbor import diamond_cubic
    from sevennet_amd.shapes import mini_sevennet_0_config
    B, K = a.B, a.steps
    pbcs = np.array([[True] * 3] * B)

    calc = _calc(sevennet_0_config(), [14])
    cells = [diamond_cubic(5.431, (2, 2, 2), 0.05, seed) for seed in range(B)]
    nums, poss, cs = [np.full(64, 14)] * B, [p for p, _ in cells], np.stack([c for _, c in cells])
    relax = lambda: calc.relax_many(nums, poss, cs, pbcs, fmax=0.0, steps=K)   # noqa: E731
    relax()   # warm-up
    if a.only_relax:
        relax()
        print(f'relax_many: B = {B}, {K} steps, info {calc.relax_info}')
        return
    print(f'per-step cost: B = {B} rattled Si 2x2x2 cells (64 atoms), SevenNet-0 shape, random weights, fmax = 0, {K} steps; '
          f'median (min .. max) of {a.reps} after warm-up')
    host_fire(calc, nums, poss, cs, pbcs, 0.0, 2)
    t_a = _timed(relax, a.reps)
    info = dict(calc.relax_info)
    t_b = _timed(lambda: host_fire(calc, nums, poss, cs, pbcs, 0.0, K), a.reps)
    t_v = _timed(lambda: host_fire_vectorised(calc, nums, poss, cs, pbcs, 0.0, K), a.reps)
    t_c = _timed(lambda: [calc.compute_many(nums, poss, cs, pbcs) for _ in range(K + 1)], a.reps)
    dpos = max(np.abs(x['positions'] - s['pos']).max() for x, s in zip(t_a[3], t_b[3][1]))
    dvec = max(np.abs(x['positions'] - q).max() for x, q in zip(t_a[3], t_v[3][1]))
    for name, t in (('(a) relax_many', t_a), ('(b) host FIRE (restatement) over compute_many', t_b),
                    ("(b') the same, numpy-vectorised over B", t_v), (f'(c) {K + 1} bare compute_many calls', t_c)):
        print(f'  {name:<46} {t[0] * 1e3:9.2f} ms ({t[1] * 1e3:.2f} .. {t[2] * 1e3:.2f})  = {t[0] * 1e3 / (K + 1):6.3f} ms per engine call')
    print(f'  all four make {K + 1} engine calls ({K} steps and the evaluation at the final positions); relax_many info {info}')
    print(f"  (b) - (a) = {(t_b[0] - t_a[0]) * 1e3 / K:.3f} ms per step, (b') - (a) = {(t_v[0] - t_a[0]) * 1e3 / K:.3f} ms per step; "
          f"(a) / (b) = {t_a[0] / t_b[0]:.3f}, "
          f"(a) / (b') = {t_a[0] / t_v[0]:.3f}")
    print(f"  largest |position difference| after {K} steps: (a) against (b) {dpos:.2e} A, (a) against (b') {dvec:.2e} A")

    calc = _calc(mini_sevennet_0_config(), [14, 8])
    rng = np.random.default_rng(0)
    sig = rng.uniform(0.02, 0.15, B)
    cells = [diamond_cubic(5.431, (2, 2, 2), float(s), seed) for seed, s in enumerate(sig)]
    nums = [np.array([14, 8])[np.random.default_rng(seed).integers(0, 2, 64)] for seed in range(B)]
    poss, cs = [p for p, _ in cells], np.stack([c for _, c in cells])
    print(f'staggered convergence: B = {B} two-species cells rattled with sigma in [0.02, 0.15], mini model, fmax = 0.02, at most 200 steps')
    for rb in (0.0, 0.5):
        run = lambda: calc.relax_many(nums, poss, cs, pbcs, fmax=0.02, steps=200, repack_below=rb)   # noqa: E731
        run()
        t = _timed(run, a.reps)
        st = [r['n_steps'] for r in t[3]]
        print(f'  relax_many repack_below = {rb}: {t[0] * 1e3:9.2f} ms ({t[1] * 1e3:.2f} .. {t[2] * 1e3:.2f}); converged '
              f'{sum(r["converged"] for r in t[3])} / {B}, steps min / median / max {min(st)} / {int(np.median(st))} / {max(st)}; {calc.relax_info}')
    host_fire(calc, nums, poss, cs, pbcs, 0.02, 2)
    t = _timed(lambda: host_fire(calc, nums, poss, cs, pbcs, 0.02, 200), a.reps)
    print(f'  host FIRE over compute_many:   {t[0] * 1e3:9.2f} ms ({t[1] * 1e3:.2f} .. {t[2] * 1e3:.2f}); converged '
          f'{sum(not s["active"] for s in t[3][1])} / {B}, engine calls {t[3][2]}, system steps evaluated {B * (t[3][2] - 1)}')


if __name__ == '__main__':
    main()
