"""GPU: the LAMMPS pair styles over the flag and rebuild sequence of a real run, on libsnet_hip.so.

tests/test_lammps_glue_gpu.py drives one `run 0`: all flags on, one neighbor list, fixed positions.  Here tests/lammps_mock/run_pair
--script walks six steps the way a run presents them to a pair style (lammps_sequence.PATTERN: everything on / nothing / thermo /
nothing + a rebuild that permutes the owned atoms and brings more ghosts / nothing / everything on), the atoms moving a little every
step, one process per style.  Every step of `e3gnn` is compared with the fp64 oracle (oracle_model(cfg, sd).forward over the
brute-force list of tests/nl_ref.py at the model cutoff, at that step's positions; 0.07 s per step for 96 atoms, so all six steps
get the oracle) at the bars of test_lammps_glue_gpu.py / test_md_host_gpu.py; the same script with all flags on at every step must
give the same bits (what the caller asks for must not change what it gets); `e3gnn/parallel` on one rank must give the serial
style's bits; `d3` is compared with D3Calculator.compute at every step's positions.  For all styles: flagless steps leave the
accumulators and per-atom arrays bit-unchanged and nothing is written behind eatom / vatom."""
import os

import numpy as np
import pytest

from helpers import load_ts_golden, oracle_model
from lammps_sequence import PATTERN, run_script, steps_of, trajectory, write_script, write_structure
from nl_ref import brute_force_list
from test_d3_cpu import NACL, RTOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, 'tests', 'lammps_mock', 'run_pair')
LMP = [0, 1, 2, 3, 5, 4]      # model xx yy zz xy yz zx -> LAMMPS xx yy zz xy xz yz
F_TOL = 1e-4                  # eV/A absolute


def _run(style, struct, script, out, style_args, coeff):
    assert os.path.exists(RUN), 'tests/lammps_mock/run_pair missing: python -m sevennet_amd.build'
    rc, res, err = run_script(RUN, style, struct, script, out, style_args, coeff)
    assert rc == 0, (rc, err[-2000:])
    return res


@pytest.fixture(scope='module')
def hfo2_runs(tmp_path_factory):
    """the three processes of the e3gnn styles and the oracle at every step's positions, computed once"""
    from sevennet_amd.model_file import write_model_file
    d, cfg, sd = load_ts_golden('hfo2_96')
    tmp = tmp_path_factory.mktemp('lmpseq')
    model = str(tmp / 'deployed.snet')
    write_model_file(model, cfg, sd)
    struct = str(tmp / 'hfo2.txt')
    write_structure(struct, d['types'] + 1, d['pos'], d['cell'], 2, skin=1.0)
    traj = trajectory(d['pos'], len(PATTERN), 0.03, seed=11)
    oracle = oracle_model(cfg, sd)
    refs = []
    for pos in traj:
        ei, ev, _, border = brute_force_list(pos, d['cell'], [True] * 3, cfg['cutoff'])
        assert len(border) == 0                      # no pair sits on the cutoff: the edge set does not depend on rounding
        out = oracle.forward(np.asarray(d['types']), ei, ev)
        refs.append({k: out[k].detach().numpy() for k in ('energy', 'forces', 'atomic_energy', 'virial', 'atomic_virial')})
    coeff = ['*', '*', model, 'Hf', 'O']
    runs = {}
    for name, style, steps in (('mixed', 'e3gnn', steps_of()), ('all_on', 'e3gnn', steps_of(all_on=True)),
                               ('parallel', 'e3gnn/parallel', steps_of(vflag_atom=False))):
        script = str(tmp / f'{name}.script')
        write_script(script, steps, traj)
        runs[name] = (steps, _run(style, struct, script, str(tmp / f'{name}.json'), [], coeff))
    return d, refs, runs


def _check_bookkeeping(steps, res):
    """all styles: the rebuild of step 4 grew nall, nothing was written behind eatom / vatom, and a flagless step changed neither
    the accumulators nor the per-atom arrays nor left a flag member set"""
    out = res['steps']
    assert len(out) == len(steps)
    assert out[3]['nall'] > out[0]['nall'], [st['nall'] for st in out]
    for s, (st, (eflag, vflag, rebuild, _, _)) in enumerate(zip(out, steps)):
        assert st['guard_ok'] and st['ago'] == (0 if rebuild else out[s - 1]['ago'] + 1), s + 1
        if eflag == 0 and vflag == 0:
            assert not st['accum_changed'] and not st['eatom_changed'] and not st['vatom_changed'], (s + 1, st['energy'], st['virial'])
            assert st['flags'] == [0] * 8, (s + 1, st['flags'])


def test_e3gnn_matches_the_fp64_oracle_on_every_step_of_the_sequence(hfo2_runs):
    d, refs, runs = hfo2_runs
    steps, res = runs['mixed']
    _check_bookkeeping(steps, res)
    n, vol = len(d['types']), res['volume']
    for s, (st, ref, (eflag, vflag, _, _, _)) in enumerate(zip(res['steps'], refs, steps)):
        f, f_ref = np.array(st['forces']), ref['forces']
        assert 1.0 < np.abs(f_ref).max() < 10.0                  # (the golden cell has max|F| = 1.9 eV/A: 1e-4 absolute is 5e-5 of it)
        assert np.abs(f - f_ref).max() <= F_TOL, (s + 1, np.abs(f - f_ref).max())
        e_ref = float(ref['energy'])
        if eflag & 1:
            assert abs(st['energy'] - e_ref) <= 1e-5 * abs(e_ref), (s + 1, st['energy'], e_ref)
        v_ref = ref['virial'][LMP]
        if vflag & 3:
            assert np.allclose(np.array(st['virial']) / vol, v_ref / vol, rtol=1e-4, atol=1e-5), (s + 1, st['virial'], v_ref)
        if eflag & 2:
            ea = np.array(st['eatom'])
            assert ea.shape == (n,) and np.abs(ea - ref['atomic_energy']).max() < 1e-4, s + 1
            assert abs(ea.sum() - st['energy']) <= 1e-6 * abs(st['energy']), (s + 1, ea.sum(), st['energy'])
        else:
            assert st['eatom'] is None
        if vflag & 4:
            va, va_ref = np.array(st['vatom']), ref['atomic_virial'][:, LMP]
            assert va.shape == (n, 6) and np.abs(va - va_ref).max() <= max(1e-6, 3e-5 * np.abs(va_ref).max()), (s + 1, np.abs(va - va_ref).max())
            # the per-atom rows are fp32 on the device (relative 6e-8 each): their sum and the fp64 global virial differ by far less
            # than the bar the rows themselves get
            vg = np.array(st['virial'])
            assert np.abs(va.sum(0) - vg).max() <= max(1e-6, 3e-5 * np.abs(vg).max()), (s + 1, va.sum(0), vg)
        else:
            assert st['vatom'] is None
    # the configurations really differ from step to step, by far more than the bar
    assert np.abs(refs[1]['forces'] - refs[0]['forces']).max() > 100 * F_TOL


def test_what_the_caller_asks_for_does_not_change_what_it_gets(hfo2_runs):
    """the same script with eflag = 3, vflag = 6 on every step: forces bit-identical step by step, and on the steps where the mixed
    run asked for a quantity, that quantity bit-identical too"""
    d, refs, runs = hfo2_runs
    steps, mixed = runs['mixed']
    _, full = runs['all_on']
    assert [st['nall'] for st in mixed['steps']] == [st['nall'] for st in full['steps']]
    for s, (a, b, (eflag, vflag, _, _, _)) in enumerate(zip(mixed['steps'], full['steps'], steps)):
        assert a['forces'] == b['forces'], s + 1
        if eflag & 1:
            assert a['energy'] == b['energy'], (s + 1, a['energy'], b['energy'])
        if vflag & 3:
            assert a['virial'] == b['virial'], (s + 1, a['virial'], b['virial'])
        if eflag & 2:
            assert a['eatom'] == b['eatom'], s + 1
        if vflag & 4:
            assert a['vatom'] == b['vatom'], s + 1
    for st in full['steps']:
        assert st['guard_ok'] and st['eatom'] is not None and st['vatom'] is not None


def test_e3gnn_parallel_on_one_rank_gives_the_serial_bits_on_every_step(hfo2_runs):
    d, refs, runs = hfo2_runs
    steps, par = runs['parallel']
    assert [st[1] for st in steps] == [2, 0, 2, 0, 0, 2]
    _check_bookkeeping(steps, par)
    _, ser = runs['mixed']
    for s, (a, b, (eflag, vflag, _, _, _)) in enumerate(zip(par['steps'], ser['steps'], steps)):
        assert a['nall'] == b['nall'] and a['forces'] == b['forces'], s + 1
        if eflag & 1:
            assert a['energy'] == b['energy'], (s + 1, a['energy'], b['energy'])


def test_d3_matches_the_calculator_on_every_step_of_the_sequence(tmp_path):
    """the NaCl cell of test_d3_cpu.py in LAMMPS' restricted triclinic frame (rotated as in test_lammps_glue_gpu.py), the same flag /
    rebuild pattern, against D3Calculator.compute at each step's positions (the library takes a cell of any orientation)"""
    from sevennet_amd.d3 import D3Calculator
    cell = np.asarray(NACL['cell'], float)
    q, l_ = np.linalg.qr(cell.T, mode='complete')
    lc = l_.T
    sg = np.sign(np.diag(lc))
    lc, q = lc * sg, q * sg
    pos0 = np.asarray(NACL['positions'], float) @ q
    struct, script = str(tmp_path / 'nacl.txt'), str(tmp_path / 'nacl.script')
    # (the style asks for no list cutoff, so the ghost shell is skin wide: 2 A holds no image of this cell, 2 A + the margin does)
    write_structure(struct, [1, 2], pos0, lc, 2, skin=2.0)
    traj = trajectory(pos0, len(PATTERN), 0.03, seed=12)
    steps = steps_of()
    write_script(script, steps, traj)
    res = _run('d3', struct, script, str(tmp_path / 'd3.json'), ['9000', '1600', 'damp_bj', 'pbe'], ['*', '*', 'Na', 'Cl'])
    _check_bookkeeping(steps, res)
    calc, seen = D3Calculator(), []
    for s, (st, pos, (eflag, vflag, _, _, _)) in enumerate(zip(res['steps'], traj, steps)):
        ref = calc.compute(NACL['numbers'], pos, lc, [True] * 3)
        f_ref = np.asarray(ref['forces'])
        assert np.abs(np.array(st['forces']) - f_ref).max() < RTOL * np.abs(f_ref).max(), s + 1
        if eflag & 1:
            assert abs(st['energy'] - ref['energy']) < RTOL * abs(ref['energy']), (s + 1, st['energy'], ref['energy'])
        if vflag & 3:
            v = np.array(st['virial'])
            stress = -v[[0, 1, 2, 5, 4, 3]] / res['volume']            # LAMMPS xx yy zz xy xz yz -> ASE Voigt xx yy zz yz xz xy
            s_ref = np.asarray(ref['stress'])
            assert np.abs(stress - s_ref).max() < RTOL * np.abs(s_ref).max(), (s + 1, stress, s_ref)
        seen.append(f_ref)
    assert np.abs(seen[5] - seen[0]).max() > 100 * RTOL * np.abs(seen[0]).max()       # (the steps really differ)
