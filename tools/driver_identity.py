#!/usr/bin/env python3
"""Bit identity of the batched drivers -- vibrations_many / phonons_many / elastic_many, relax_many, md_many, neb_many -- between
two trees of this package (a refactor of their host code or of their kernels against its parent commit).

    python tools/driver_identity.py TREE OUT.pkl [--only relax_many,md_many]    run the calls below (or those of the named
                                                             methods only) with the package of TREE, pickle the results
    python tools/driver_identity.py --compare A.pkl B.pkl [--report FILE]    A is the reference

Each tree runs in a process of its own, on the libsnet_hip.so built in it (both may share one through SNET_HIP_LIB when no
kernel differs).  Inputs: tests/helpers.py three_small_systems (seed 0); its periodic system and two rattled periodic cells of 2
and 3 atoms (`crystals`) where every system must be periodic; mini SevenNet-0 shape, random weights seed 0, species Si / O.
Calls: vibrations_many with nfree 2 and 4, all atoms or `indices` for one system, one call or several (max_atoms_per_call);
phonons_many (supercell (2,1,1)) with a 3-point path, a 2x1x1 mesh, two temperatures and max_q_per_call = 1; elastic_many clamped
and with relax_ions; these with and without the per-atom virial.  relax_many (fmax 0.02, 200 steps) with repack_below 0.5 and 0,
and with relax_cell (fmax 1e-4) on the crystals; md_many (1 fs, 20 steps, 300 K, seed 0, traj_every 5) with friction 0 and 0.01, and with
pressure 0 / compressibility 60 on the crystals; neb_many (fmax 1e-4, 50 steps), plain and climbing, on a band of 3 moving images between two rattles
of the periodic system.  Each on SevenNetCalculator and on SevenNetD3Calculator with d3_term 'device' and, where it is allowed,
'host'.  A call that raises is recorded by its exception.  Compared: every key of every result dict -- arrays by shape, dtype and
np.array_equal with NaN equal to NaN, everything else by == and type -- and the info counters by ==."""
import argparse
import os
import pickle
import sys

import numpy as np

Z = [14, 8]
MASS = {14: 28.0855, 8: 15.999}
D3_CUT = dict(vdw_cutoff=1600.0, cn_cutoff=900.0)
BUDGETS = {'one call': 32768, 'several calls': 20}


def crystals(three):
    """the periodic system of `three` and two rattled triclinic cells of 2 and 3 atoms"""
    rng = np.random.default_rng(0)
    out = [three[0]]
    for n, cell in ((2, [[4.0, 0.0, 0.0], [0.3, 4.2, 0.0], [0.2, 0.1, 4.4]]), (3, [[4.6, 0.0, 0.0], [-0.2, 4.1, 0.0], [0.1, 0.3, 4.3]])):
        frac = (np.arange(n)[:, None] + np.array([0.1, 0.2, 0.3])) / n
        out.append((rng.integers(0, 2, n), frac @ np.array(cell) + rng.normal(0, 0.05, (n, 3)), np.array(cell), [True] * 3))
    return out


def cases(three):
    """(name, method, info attribute, arguments, keywords, d3_term 'host' allowed, run with the per-atom virial on too)"""
    num = lambda s: [np.array(Z)[t] for t, _, _, _ in s]   # noqa: E731
    mass = lambda s: [np.array([MASS[z] for z in zz]) for zz in num(s)]   # noqa: E731
    geo = lambda s: (np.stack([c for _, _, c, _ in s]), np.array([p for _, _, _, p in s]))   # noqa: E731
    cry = crystals(three)
    for nfree in (2, 4):
        for idx_name, idx in (('all atoms', None), ('indices for system 1', [None, [0, 2, 3], None])):
            for b_name, budget in BUDGETS.items():
                yield (f'vibrations_many(nfree={nfree}, {idx_name}, {b_name})', 'vibrations_many', 'vib_info',
                       (num(three), [p for _, p, _, _ in three], mass(three)) + geo(three),
                       dict(nfree=nfree, indices=idx, max_atoms_per_call=budget), True, True)
    path = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.5, 0.0, 0.0]])
    for b_name, budget in BUDGETS.items():
        yield (f'phonons_many(path 3, mesh 2x1x1, 2 temperatures, max_q_per_call=1, {b_name})', 'phonons_many', 'phonon_info',
               (num(cry), [p for _, p, _, _ in cry], mass(cry)) + geo(cry) + ((2, 1, 1),),
               dict(qpoints=path, mesh=(2, 1, 1), temperatures=[0.0, 300.0], max_q_per_call=1, max_atoms_per_call=budget, want_modes=True), True, True)
        for relax_ions in (False, True):
            yield (f'elastic_many(relax_ions={relax_ions}, {b_name})', 'elastic_many', 'elastic_info',
                   (num(cry), [p for _, p, _, _ in cry]) + geo(cry), dict(relax_ions=relax_ions, max_atoms_per_call=budget), False, True)
    pos = lambda s: [p for _, p, _, _ in s]   # noqa: E731
    for repack in (0.5, 0):
        yield (f'relax_many(repack_below={repack})', 'relax_many', 'relax_info', (num(three), pos(three)) + geo(three),
               dict(fmax=0.02, steps=200, repack_below=repack), True, False)
    yield ('relax_many(relax_cell=True)', 'relax_many', 'relax_info', (num(cry), pos(cry)) + geo(cry),
           dict(fmax=1e-4, steps=200, relax_cell=True), False, False)   # (the model's forces alone are below 0.02)
    md = dict(dt=1.0, steps=20, temperature=300.0, seed=0, traj_every=5)
    for friction in (0.0, 0.01):
        yield (f'md_many(friction={friction})', 'md_many', 'md_info', (num(three), pos(three), mass(three)) + geo(three),
               dict(md, friction=friction), True, False)
    yield ('md_many(pressure=0.0, compressibility=60.0)', 'md_many', 'md_info', (num(cry), pos(cry), mass(cry)) + geo(cry),
           dict(md, friction=0.01, pressure=0.0, compressibility=60.0), False, False)
    t, p0, cell, pbc = three[0]   # the periodic system: a band of 3 moving images between two rattles of it
    rng = np.random.default_rng(1)
    ends = [p0 + rng.normal(0, 0.05, p0.shape) for _ in range(2)]
    band = ends[0][None] + np.linspace(0.0, 1.0, 5)[:, None, None] * (ends[1] - ends[0])[None]
    for climb in (False, True):
        yield (f'neb_many(climb={climb})', 'neb_many', 'neb_info', ([np.array(Z)[t]], [band], np.array(cell)[None], np.array([pbc])),
               dict(fmax=1e-4, steps=50, climb=climb), True, False)


def run(tree, out_path, only=None):
    sys.path.insert(0, os.path.abspath(tree))
    sys.path.insert(0, os.path.join(os.path.abspath(tree), 'tests'))
    import sevennet_amd
    from helpers import three_small_systems
    from sevennet_amd.calculator import SevenNetCalculator
    from sevennet_amd.d3 import SevenNetD3Calculator
    from sevennet_amd.shapes import mini_sevennet_0_config
    from sevennet_amd.synthetic import random_state_dict
    assert os.path.abspath(sevennet_amd.__file__).startswith(os.path.abspath(tree) + os.sep), sevennet_amd.__file__
    cfg = dict(mini_sevennet_0_config(), _type_map={z: k for k, z in enumerate(Z)})
    model = (cfg, random_state_dict(cfg, seed=0))
    snet = SevenNetCalculator(model, file_type='model_instance', device='cuda:0')
    d3 = SevenNetD3Calculator(model, file_type='model_instance', device='cuda:0', **D3_CUT)
    three = three_small_systems(0)
    record = {}
    for atomic_virial in (False, True):
        snet.compute_atomic_virial = d3.calcs[0].compute_atomic_virial = atomic_virial
        for name, method, info, args, kw, host_allowed, both_virials in cases(three):
            if (atomic_virial and not both_virials) or (only and method not in only):
                continue
            for calc_name, calc, extra in (('snet', snet, {}), ('snet_d3[device]', d3, dict(d3_term='device')), ('snet_d3[host]', d3, dict(d3_term='host'))):
                if calc is d3 and extra['d3_term'] == 'host' and not host_allowed:
                    continue
                key = f'{calc_name}.{name}, atomic virial {"on" if atomic_virial else "off"}'
                try:
                    record[key] = (getattr(calc, method)(*args, **kw, **extra), dict(getattr(calc, info)))
                except Exception as e:   # (recorded: both trees must raise the same)
                    record[key] = repr(e)
                print(key, '->', record[key] if isinstance(record[key], str) else record[key][1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'wb') as f:
        pickle.dump(record, f)


def differences(a, b, where):
    """the places where b is not a, bit for bit"""
    if type(a) is not type(b):
        return [f'{where}: {type(a).__name__} against {type(b).__name__}']
    if isinstance(a, dict):
        out = [] if list(a) == list(b) else [f'{where}: keys {list(a)} against {list(b)}']
        return out + [d for k in a if k in b for d in differences(a[k], b[k], f'{where}[{k!r}]')]
    if isinstance(a, (list, tuple)):
        out = [] if len(a) == len(b) else [f'{where}: length {len(a)} against {len(b)}']
        return out + [d for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, f'{where}[{i}]')]
    if isinstance(a, np.ndarray):
        same = a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind in 'fc')
        return [] if same else [f'{where}: arrays {a.shape} {a.dtype} against {b.shape} {b.dtype} differ']
    same = a == b or (isinstance(a, float) and a != a and b != b)
    return [] if same else [f'{where}: {a!r} against {b!r}']


def compare(ref_path, new_path, report):
    with open(ref_path, 'rb') as f:
        ref = pickle.load(f)
    with open(new_path, 'rb') as f:
        new = pickle.load(f)
    lines, bad = [], list(differences(list(ref), list(new), 'the calls'))
    for key, want in ref.items():
        lines.append(key)
        if isinstance(want, str):
            lines.append(f'    raises {want}')
        else:
            arrays = {k: [r[k].shape for r in want[0]] for k, v in want[0][0].items() if isinstance(v, np.ndarray)}
            other = {k: [r[k] for r in want[0]] for k, v in want[0][0].items() if isinstance(v, (bool, int, str))}
            lines += [f'    info {want[1]}', f'    arrays per system {arrays}', f'    {other}']
        diff = differences(want, new.get(key), key)
        bad += diff
        lines += [f'    DIFFERS {d}' for d in diff] or ['    -> identical']
    lines.append('ALL IDENTICAL' if not bad else f'{len(bad)} DIFFERENCES')
    print('\n'.join(lines))
    if report:
        with open(report, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('paths', nargs=2, help='TREE OUT.pkl, or with --compare: REFERENCE.pkl NEW.pkl')
    ap.add_argument('--compare', action='store_true')
    ap.add_argument('--report')
    ap.add_argument('--only', help='comma-separated method names: run only the calls of these')
    a = ap.parse_args()
    sys.exit(compare(a.paths[0], a.paths[1], a.report) if a.compare else run(*a.paths, only=a.only.split(',') if a.only else None))


if __name__ == '__main__':
    main()
