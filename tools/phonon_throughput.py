#!/usr/bin/env python3
"""Cost of batched supercell phonons (SevenNetCalculator.phonons_many) against the same rule on the host.

  workload   B diamond-structure Si primitive cells (2 atoms, lattice constants spread over 2 %), repeats (3,3,3): 54-atom
             supercells, nfree = 2: 13 copies per cell; a q-path of --path points and a Gamma-centred --mesh^3 mesh, SevenNet-0 shape
  (a)        phonons_many
  (a')       phonons_many with the device synchronised around every snet_ph_dynmat call: its D(q) share (not a timing of (a))
  (b)        the same copies built on the host and sent through compute_many in chunks of the same atom budget, the forces brought
             down; Phi, the sum rule, the 27-candidate images and D(q) in numpy (the rule of include/snet_hip.h, vectorised), the
             same eigh and thermodynamics; its D(q) share is timed on the host

Device-synchronised wall clock after warm-up; the legs are interleaved ((a), (a'), (b), (a), ...) in one process on one device,
median of --reps.  The report goes to stdout and to --out.

    python tools/phonon_throughput.py [--reps 3] [--B 24] [--mesh 8] [--path 101] [--budget 32768] [--out profiles/phonon_throughput.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DELTA, NFREE, MASS_SI, REPEATS, SYMPREC = 0.01, 2, 28.0855, (3, 3, 3), 1e-5


def _calc(cfg, z):
    from sevennet_amd.calculator import SevenNetCalculator
    from sevennet_amd.synthetic import random_state_dict
    cfg = dict(cfg, _type_map={zz: k for k, zz in enumerate(z)})
    return SevenNetCalculator((cfg, random_state_dict(cfg, 0)), file_type='model_instance', device='cuda:0')


def make_cells(B):
    """[(numbers, positions, cell)]: fcc primitive cells of the diamond structure, a = 5.431 A (1 + up to 2 %), slightly rattled"""
    rng = np.random.default_rng(0)
    out = []
    for b in range(B):
        a = 5.431 * (1.0 + 0.02 * b / max(B - 1, 1))
        cell = 0.5 * a * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
        out.append((np.array([14, 14]), np.array([[0.0, 0.0, 0.0], [a / 4, a / 4, a / 4]]) + rng.normal(0.0, 0.01, (2, 3)), cell))
    return out


# ------------------------------------------------------------------------------------------------ the rule on the host
def host_images(pos, S, m):
    """the 27 candidates around the wrapped pair -> d [m,N,27,3] and the weights [m,N,27] (1 / n_kept on the kept ones)"""
    d0 = pos[None, :, :] - pos[:m, None, :]
    n0 = -np.rint(d0 @ np.linalg.inv(S))
    shifts = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing='ij'), -1).reshape(27, 3)
    d = d0[:, :, None, :] + (n0[:, :, None, :] + shifts[None, None]) @ S
    length = np.sqrt((d * d).sum(-1))
    keep = length <= length.min(-1, keepdims=True) + SYMPREC
    return d, keep / keep.sum(-1, keepdims=True)


def host_dynmat(phi, pos, S, m, masses, q_cart):
    """D(q) [n_q,3m,3m] from Phi [m,N,3,3]"""
    N = len(pos)
    d, wgt = host_images(pos, S, m)
    phase = (np.exp(1j * np.einsum('qx,ajtx->qajt', q_cart, d)) * wgt[None]).sum(-1)              # [n_q,m,N]
    w = 1.0 / np.sqrt(masses)
    R = np.einsum('acbik,qacb->qaibk', phi.reshape(m, N // m, m, 3, 3), phase.reshape(len(q_cart), m, N // m, m))
    R = (R * (w[:, None, None, None] * w[None, None, :, None])[None]).reshape(len(q_cart), 3 * m, 3 * m)
    return 0.5 * (R + np.conj(np.swapaxes(R, 1, 2)))


def host_phonons(calc, systems, q_frac, n_path, temps, budget):
    """(b) -> (per system: Phi, path energies, thermo), engine calls, seconds spent in D(q)"""
    from sevennet_amd.phonon import build_supercell, spectrum, thermodynamics
    sc = [build_supercell(z, pos, cell, REPEATS) for z, pos, cell in systems]
    copies = []
    for b, (z, pos, S) in enumerate(sc):
        for a in range(2):
            for i in range(3):
                for q in (-1, 1):
                    p = pos.copy()
                    p[a, i] = p[a, i] + float(q) * DELTA
                    copies.append((b, p))
        copies.append((b, pos))
    per = max(1, budget // len(sc[0][1]))
    forces, calls = [], 0
    for c0 in range(0, len(copies), per):
        chunk = copies[c0:c0 + per]
        res = calc.compute_many([sc[b][0] for b, _ in chunk], [p for _, p in chunk], np.stack([sc[b][2] for b, _ in chunk]), [True] * 3)
        forces += [r['forces'] for r in res]
        calls += 1
    out, j, t_dyn = [], 0, 0.0
    for b, (z, pos, S) in enumerate(sc):
        N = len(pos)
        phi = np.stack([(forces[j + 2 * r] - forces[j + 2 * r + 1]) / (2.0 * DELTA) for r in range(6)]).reshape(2, 3, N, 3).transpose(0, 2, 1, 3).copy()
        j += 13
        for a in range(2):   # the acoustic sum rule on the self terms
            phi[a, a] = 0.0
            phi[a, a] = -phi[a].sum(0)
        t0 = time.perf_counter()
        D = host_dynmat(phi, pos, S, 2, np.full(2, MASS_SI), 2.0 * np.pi * (q_frac @ np.linalg.inv(systems[b][2]).T))
        t_dyn += time.perf_counter() - t0
        e = spectrum(D)['energies']
        out.append((phi, e[:n_path], thermodynamics(e[n_path:], temps)))
    return out, calls, t_dyn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--B', type=int, default=24)
    ap.add_argument('--mesh', type=int, default=8)
    ap.add_argument('--path', type=int, default=101)
    ap.add_argument('--budget', type=int, default=32768)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'phonon_throughput.txt'))
    a = ap.parse_args()
    import torch
    from sevennet_amd import phonon
    from sevennet_amd.model_spec import sevennet_0_config
    calc = _calc(sevennet_0_config(), [14])
    systems = make_cells(a.B)
    path = phonon.band_path([[0.0, 0.0, 0.0], [0.5, 0.0, 0.5], [0.5, 0.25, 0.75], [0.375, 0.375, 0.75], [0.0, 0.0, 0.0], [0.5, 0.5, 0.5]],
                            max(1, (a.path - 1) // 5))
    mesh, temps = (a.mesh,) * 3, [0.0, 300.0, 1000.0]
    q_frac = np.concatenate([path, phonon.mesh_points(mesh)])
    args = ([z for z, _, _ in systems], [p for _, p, _ in systems], [np.full(2, MASS_SI)] * a.B, np.stack([c for _, _, c in systems]), [True] * 3)
    kw = dict(qpoints=path, mesh=mesh, temperatures=temps, delta=DELTA, nfree=NFREE, max_atoms_per_call=a.budget)
    dyn = {'t': 0.0, 'n': 0}
    plain_dynmat = phonon.ph_dynmat

    def timed_dynmat(*x):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plain_dynmat(*x)
        torch.cuda.synchronize()
        dyn['t'] += time.perf_counter() - t0
        dyn['n'] += 1

    def leg_a_split():
        dyn['t'], dyn['n'] = 0.0, 0
        phonon.ph_dynmat = timed_dynmat
        try:
            return calc.phonons_many(*args, REPEATS, **kw), dyn['t']
        finally:
            phonon.ph_dynmat = plain_dynmat

    legs = {'(a) phonons_many': lambda: calc.phonons_many(*args, REPEATS, **kw),
            "(a') phonons_many, D(q) calls synchronised": leg_a_split,
            '(b) host copies over chunked compute_many, numpy': lambda: host_phonons(calc, systems, q_frac, len(path), temps, a.budget)}
    calc.phonons_many(*[x[:2] for x in args[:4]], [True] * 3, REPEATS, **kw)   # warm-up on two cells
    host_phonons(calc, systems[:1], q_frac, len(path), temps, a.budget)
    times, last = {name: [] for name in legs}, {}
    for _ in range(a.reps):   # interleaved: each repetition runs every leg once
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    info = dict(calc.phonon_info)
    names = list(legs)
    n_q = len(q_frac)
    lines = [f'supercell phonons: B = {a.B} Si primitive cells (2 atoms), repeats {REPEATS} (54-atom supercells), nfree = {NFREE}, delta = {DELTA} A: '
             f'{a.B * 13} copies, {len(path)} path + {a.mesh}^3 mesh = {n_q} q-points per cell, SevenNet-0 shape, random weights, at most '
             f'{a.budget} atoms per call; legs interleaved, median (min .. max) of {a.reps} after warm-up']
    med = {}
    for name, ts in times.items():
        med[name] = float(np.median(ts))
        lines.append(f'  {name:<52} {med[name] * 1e3:10.2f} ms ({min(ts) * 1e3:.2f} .. {max(ts) * 1e3:.2f})')
    ta, tb = med[names[0]], med[names[2]]
    res_a, (res_b, calls_b, dyn_b) = last[names[0]], last[names[2]]
    dyn_a = last[names[1]][1]
    d_phi = max(np.abs(r['force_constants'] - h[0]).max() for r, h in zip(res_a, res_b))
    d_e = max(np.abs(r['energies'] - h[1]).max() for r, h in zip(res_a, res_b))
    d_f = max(np.abs(r['thermo']['free_energy'] - h[2]['free_energy']).max() for r, h in zip(res_a, res_b))
    lines.append(f"  D(q) share: (a') {dyn_a * 1e3:.2f} ms in {dyn['n']} snet_ph_dynmat call(s) for {info['q_evaluated']} q-points (last "
                 f'repetition, device synchronised around them); (b) {dyn_b * 1e3:.2f} ms in numpy (last repetition)')
    lines.append(f'  (a) makes {info["n_force_calls"]} engine calls, (b) {calls_b}; phonons_many info {info}')
    lines.append(f'  (a) / (b) = {ta / tb:.3f}; largest difference (a) against (b): force constants {d_phi:.2e} eV/A^2, path energies {d_e:.2e} eV, '
                 f'free energies {d_f:.2e} eV')
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
