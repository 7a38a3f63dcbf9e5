"""Test helper: scripts for `tests/lammps_mock/run_pair --script` (the flag / rebuild sequence of a real LAMMPS run) and the
runner shared by tests/test_lammps_sequence_cpu.py (glue against the recording stand-in tests/lammps_mock/snet_stub.cpp) and
tests/test_lammps_sequence_gpu.py (the same sequence on libsnet_hip.so)."""
import json
import subprocess

import numpy as np

# (eflag, vflag, rebuild): a step with everything on, an ordinary MD step, a thermo step (global energy + virial), a rebuild on
# an ordinary step (permuted local order, more ghosts), an ordinary step on the new list, a dump step on the new list
PATTERN = ((3, 6, 1), (0, 0, 0), (1, 2, 0), (0, 0, 1), (0, 0, 0), (3, 6, 0))
# the rebuild that grows nall directly after a step with per-atom output: a style that still believes in that step's flags writes
# eatom[nall] / vatom[nall, 6] of the NEW nall into arrays sized by the old one
GROW_AFTER_PER_ATOM = ((3, 6, 1), (0, 0, 1), (0, 0, 0), (3, 6, 0))
REBUILD_MARGIN = 1.5      # A added to cutoff + skin at the rebuild of step 4: nall must come out strictly larger than at step 1
FLAG_NAMES = ('eflag_either', 'eflag_global', 'eflag_atom', 'vflag_either', 'vflag_global', 'vflag_atom', 'evflag', 'vflag_fdotr')


def write_structure(path, types1, pos, cell, ntypes, skin):
    with open(path, 'w') as f:
        f.write(f'{len(pos)} {ntypes}\n')
        for row in np.asarray(cell, float):
            f.write(' '.join(repr(float(v)) for v in row) + '\n')
        f.write(f'{skin}\n')
        for t, p in zip(types1, np.asarray(pos, float)):
            f.write(f'{int(t)} ' + ' '.join(repr(float(v)) for v in p) + '\n')


def trajectory(pos, n_steps, max_step, seed):
    """positions of every step: the given ones plus a cumulative uniform displacement of at most max_step per component per step"""
    rng = np.random.default_rng(seed)
    pos = np.asarray(pos, float)
    out = [pos.copy()]
    for _ in range(n_steps - 1):
        out.append(out[-1] + rng.uniform(-max_step, max_step, pos.shape))
    return out


def steps_of(pattern=PATTERN, vflag_atom=True, all_on=False):
    """[(eflag, vflag, rebuild, perm_seed, ghost_margin)]: the first rebuild keeps tag order and no margin, every later one
    permutes the owned atoms and adds REBUILD_MARGIN; all_on asks for everything on every step of the same sequence"""
    out = []
    for s, (e, v, rb) in enumerate(pattern):
        if all_on:
            e, v = pattern[0][0], pattern[0][1]
        if not vflag_atom:
            v &= ~4
        out.append((e, v, rb, 0 if s == 0 else 1000 + s, 0.0 if s == 0 else REBUILD_MARGIN) if rb else (e, v, 0, 0, 0.0))
    return out


def write_script(path, steps, positions):
    with open(path, 'w') as f:
        for (e, v, rb, seed, margin), pos in zip(steps, positions):
            f.write(f'{e} {v} {rb} {seed} {margin!r}\n')
            for p in np.asarray(pos, float):
                f.write(' '.join(repr(float(x)) for x in p) + '\n')


def run_script(exe, style, struct, script, out, style_args, coeff, env=None, timeout=600):
    """-> (returncode, parsed output or None, stderr)"""
    r = subprocess.run([exe, style, struct, out, '--script', script] + list(style_args) + ['--'] + list(coeff), capture_output=True,
                       text=True, timeout=timeout, env=env)
    res = None
    if r.returncode in (0, 4, 5):
        with open(out) as f:
            res = json.load(f)
    return r.returncode, res, r.stderr


def flags_of(step):
    return dict(zip(FLAG_NAMES, step['flags']))
