"""CPU: the LAMMPS pair styles over the flag and rebuild sequence of a real run, against a recording stand-in for the library.

lammps/pair_e3gnn_hip.cpp and lammps/pair_d3_hip.cpp are compiled with the scripted mock driver (tests/lammps_mock/run_pair.cpp
--script) and tests/lammps_mock/snet_stub.cpp -- every C-ABI function the two sources call, no GPU, each call logged as one JSON
line -- into a stand-alone executable with -fsanitize=address,undefined, and run directly.  The script is what a run looks like
to a pair style: almost every step eflag = vflag = 0, a thermo step, a dump step, a neighbor-list rebuild in between that permutes
the owned atoms and grows nall.  Checked: what the glue hands to snet_md_compute on every step, that flagless steps leave the
accumulators, the per-atom arrays and the flag members as stock ev_init / ev_unset would, that nothing is written behind eatom /
vatom (guard bands of the mock's ev_setup, and the sanitizer where it links)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from lammps_sequence import GROW_AFTER_PER_ATOM, PATTERN, flags_of, run_script, steps_of, trajectory, write_script, write_structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, 'tests', 'lammps_mock')
HIP_INCLUDE = '/opt/rocm/include'
GLUE = [os.path.join(ROOT, 'lammps', 'pair_e3gnn_hip.cpp'), os.path.join(ROOT, 'lammps', 'pair_d3_hip.cpp')]

pytestmark = pytest.mark.skipif(shutil.which('g++') is None or not os.path.exists(os.path.join(HIP_INCLUDE, 'hip', 'hip_runtime.h')),
                                reason='needs g++ and the HIP headers')

LIBRARY_CALL = r'\b(snet_[a-z0-9_]+|pair_(?:init|failed|set_atom|set_domain|run_settings|run_coeff|run_compute|get_energy|get_force|get_stress|fin)|hip[A-Z][A-Za-z]+)\('
SANITIZER_REPORT = ('AddressSanitizer', 'runtime error:', 'LeakSanitizer')


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    """(executable, built with the sanitizers?)"""
    tmp = tmp_path_factory.mktemp('lmpseq')
    exe = str(tmp / 'run_pair_stub')
    srcs = [os.path.join(MOCK, 'run_pair.cpp'), os.path.join(MOCK, 'lmp_mock_runtime.cpp'), os.path.join(MOCK, 'snet_stub.cpp')] + GLUE
    base = ['g++', '-std=c++17', '-O1', '-g', '-D__HIP_PLATFORM_AMD__', f'-I{MOCK}', '-I' + os.path.join(ROOT, 'include'), f'-I{HIP_INCLUDE}']
    san = ['-fsanitize=address,undefined', '-fno-omit-frame-pointer']
    # the static runtimes first: a stand-alone executable that carries its sanitizer starts under any environment; then the shared
    # ones; then no sanitizer (the guard bands still check the per-atom arrays).  A build counts only if the executable starts.
    for extra in (san + ['-static-libasan', '-static-libubsan'], san, []):
        r = subprocess.run(base + extra + srcs + ['-o', exe], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            # only a sanitizer runtime that is not installed is excused
            assert extra and re.search(r'sanitize|asan|ubsan', r.stderr), r.stderr[-3000:]
            continue
        started = subprocess.run([exe], capture_output=True, text=True)
        if started.returncode == 2 and 'usage: run_pair' in started.stderr:
            return exe, bool(extra)
        assert extra, (started.returncode, started.stderr[-3000:])
    raise AssertionError('the stub harness could not be built')


@pytest.fixture(scope='module')
def system(tmp_path_factory):
    """8 atoms of two types in a 6 A cube (stub cutoff 4.0 + skin 1.0: 62 ghosts, 1.5 A more margin doubles them), six steps of small moves"""
    tmp = tmp_path_factory.mktemp('lmpseq_in')
    rng = np.random.default_rng(0)
    cell = np.diag([6.0, 6.0, 6.0])
    frac = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75], [.75, .75, .25]])
    pos = frac @ cell + rng.uniform(-0.1, 0.1, (8, 3)) + 0.3
    types1 = [1, 2, 2, 1, 2, 1, 1, 2]
    struct = str(tmp / 'cube.txt')
    write_structure(struct, types1, pos, cell, 2, skin=1.0)
    return struct, trajectory(pos, len(PATTERN), 0.03, seed=1), tmp


def _run(harness, system, style, steps, name, style_args=(), coeff=('*', '*', 'stub.snet', 'Hf', 'O'), positions=None):
    exe, _ = harness
    struct, traj, tmp = system
    script, out, log = str(tmp / f'{name}.script'), str(tmp / f'{name}.json'), str(tmp / f'{name}.log')
    write_script(script, steps, traj if positions is None else positions)
    env = dict(os.environ, SNET_STUB_LOG=log)
    rc, res, err = run_script(exe, style, struct, script, out, list(style_args), list(coeff), env=env)
    calls = [json.loads(ln) for ln in open(log)] if os.path.exists(log) else []
    return rc, res, err, calls


def _clean(rc, err):
    assert rc == 0, (rc, err[-3000:])
    assert not any(s in err for s in SANITIZER_REPORT), err[-3000:]


def test_the_stub_defines_every_library_function_the_glue_calls(harness):
    """the list comes from the pair sources themselves (as in test_lammps_glue_cpu.py); the link of the harness proves the same"""
    stub = open(os.path.join(MOCK, 'snet_stub.cpp')).read()
    called = set()
    for src in GLUE:
        called |= set(re.findall(LIBRARY_CALL, open(src).read()))
    assert {'snet_md_compute', 'snet_md_list_unchanged', 'snet_halo_create', 'pair_run_compute', 'hipStreamCreateWithFlags'} <= called
    for fn in sorted(called):
        assert re.search(r'^[A-Za-z_][\w \*]*\b' + fn + r'\(', stub, flags=re.M), fn


def _check_flagged_and_flagless(res, steps, per_atom_value=None):
    """what every style owes LAMMPS: flagless steps change nothing but f and leave the flags as ev_unset would; a flagged step
    holds ONE energy (the stub's 1.0) and ONE virial (1 .. 6), nothing carried over"""
    out = res['steps']
    assert len(out) == len(steps)
    for s, (st, (eflag, vflag, rebuild, _, _)) in enumerate(zip(out, steps)):
        where = f'step {s + 1} (eflag {eflag}, vflag {vflag}, rebuild {rebuild})'
        assert st['guard_ok'], where
        assert st['ago'] == (0 if rebuild else out[s - 1]['ago'] + 1), where
        if eflag == 0 and vflag == 0:
            assert not st['accum_changed'], (where, st['energy'], st['virial'])
            assert not st['eatom_changed'] and not st['vatom_changed'], where
            assert st['flags'] == [0] * 8, (where, flags_of(st))
            assert st['eatom'] is None and st['vatom'] is None
        else:
            assert st['energy'] == (1.0 if eflag & 1 else 0.0), (where, st['energy'])
            assert st['virial'] == ([1.0, 2.0, 3.0, 4.0, 5.0, 6.0] if vflag & 3 else [0.0] * 6), (where, st['virial'])
            fl = flags_of(st)
            assert (fl['eflag_global'], fl['eflag_atom'], fl['vflag_atom']) == (eflag & 1, int(bool(eflag & 2)), int(bool(vflag & 4))), where
            assert bool(fl['vflag_global']) == bool(vflag & 3) and fl['evflag'] == 1, where
            if per_atom_value is not None:
                e_val, v_val = per_atom_value
                assert (st['eatom'] is not None) == bool(eflag & 2) and (st['vatom'] is not None) == bool(vflag & 4), where
                if eflag & 2:
                    assert st['eatom'] == [e_val] * res['nlocal'], where
                if vflag & 4:
                    assert st['vatom'] == [[v_val] * 6] * res['nlocal'], where


def test_e3gnn_asks_the_library_only_for_what_the_step_asks(harness, system):
    steps = steps_of()
    rc, res, err, calls = _run(harness, system, 'e3gnn', steps, 'serial')
    _clean(rc, err)
    out = res['steps']
    assert out[3]['nall'] > out[0]['nall'], [st['nall'] for st in out]        # the rebuild of step 4 grew nall
    assert out[1]['nall'] == out[2]['nall'] == out[0]['nall'] and out[4]['nall'] == out[5]['nall'] == out[3]['nall']
    mdc = [c for c in calls if c['fn'] == 'snet_md_compute']
    assert len(mdc) == len(steps)
    for s, (c, st, (eflag, vflag, rebuild, _, _)) in enumerate(zip(mdc, out, steps)):
        where = f'step {s + 1} (eflag {eflag}, vflag {vflag}, rebuild {rebuild}): {c}'
        assert c['nall'] == st['nall'] and c['inum'] == res['nlocal'] and c['ghost_mode'] == 0, where
        assert c['eflag_atom'] == int(bool(eflag & 2)) and c['vflag_atom'] == int(bool(vflag & 4)), where
        assert bool(c['vflag']) == bool(vflag), where
        assert c['eatom_null'] == int(not eflag & 2) and c['vatom_null'] == int(not vflag & 4), where
        assert c['f_null'] == 0 and c['stream_null'] == 0, where
        assert c['list_unchanged'] == int(not rebuild), where                  # the hint on exactly the non-rebuild steps
    assert sum(c['fn'] == 'snet_md_list_unchanged' for c in calls) == sum(not st[2] for st in steps)
    _check_flagged_and_flagless(res, steps, per_atom_value=(0.125, 0.0625))
    # forces are added on every step: 0.5 per component for the atom and for each of its ghost images, folded by the driver
    for st in out:
        f = np.array(st['forces'])
        assert (f >= 1.0).all() and (f % 0.5 == 0).all() and (f == f[:, :1]).all()
    assert np.array(out[3]['forces']).sum() > np.array(out[0]['forces']).sum()        # more images after the rebuild


def test_e3gnn_does_not_write_per_atom_arrays_of_an_earlier_step_after_nall_grew(harness, system):
    """the list is rebuilt, with more ghosts, on the flagless step right after a dump step: eatom / vatom still have the size of
    the dump step's ev_setup and must not be touched (guard bands; a heap-buffer-overflow report where the sanitizer runs)"""
    steps = steps_of(GROW_AFTER_PER_ATOM)
    rc, res, err, calls = _run(harness, system, 'e3gnn', steps, 'grow')
    _clean(rc, err)
    grown = res['steps'][1]['nall'] - res['steps'][0]['nall']
    assert grown > 0 and 6 * grown > 64, [st['nall'] for st in res['steps']]     # vatom would be overrun past its guard band too
    _check_flagged_and_flagless(res, steps, per_atom_value=(0.125, 0.0625))
    for c, (eflag, vflag, _, _, _) in zip([c for c in calls if c['fn'] == 'snet_md_compute'], steps):
        assert c['eatom_null'] == int(not eflag & 2) and c['vatom_null'] == int(not vflag & 4), c


def test_e3gnn_parallel_rebuilds_its_halo_plan_with_the_list_only(harness, system):
    steps = steps_of(vflag_atom=False)
    assert [st[1] for st in steps] == [2, 0, 2, 0, 0, 2]
    rc, res, err, calls = _run(harness, system, 'e3gnn/parallel', steps, 'parallel')
    _clean(rc, err)
    _check_flagged_and_flagless(res, steps)
    # between two snet_md_compute calls: snet_md_nodes + snet_halo_create + snet_model_set_rccl_halo iff the step rebuilt the list
    per_step, cur = [], []
    for c in calls:
        if c['fn'] == 'snet_md_compute':
            per_step.append((cur, c))
            cur = []
        elif c['fn'] in ('snet_halo_create', 'snet_md_nodes', 'snet_model_set_rccl_halo', 'snet_md_list_unchanged', 'snet_halo_destroy'):
            cur.append(c['fn'])
    assert len(per_step) == len(steps)
    for s, ((before, c), (eflag, vflag, rebuild, _, _)) in enumerate(zip(per_step, steps)):
        assert before.count('snet_halo_create') == before.count('snet_md_nodes') == before.count('snet_model_set_rccl_halo') == rebuild, (s + 1, before)
        assert before.count('snet_md_list_unchanged') == int(not rebuild), (s + 1, before)
        assert before.count('snet_halo_destroy') == (1 if rebuild and s > 0 else 0), (s + 1, before)
        assert c['ghost_mode'] == 1 and c['vflag_atom'] == 0 and c['vatom_null'] == 1, (s + 1, c)
        assert c['eflag_atom'] == int(bool(eflag & 2)) and c['eatom_null'] == int(not eflag & 2), (s + 1, c)
        assert bool(c['vflag']) == bool(vflag), (s + 1, c)
    # per-atom stress is refused by the style itself, on the step that asks for it
    bad = list(steps)
    bad[2] = (1, 6, 0, 0, 0.0)
    rc, res, err, calls = _run(harness, system, 'e3gnn/parallel', bad, 'parallel_vatom')
    assert rc == 3 and 'atomic stress is not supported' in err, (rc, err[-2000:])
    assert sum(c['fn'] == 'snet_md_compute' for c in calls) == 2
    assert not any(s in err for s in SANITIZER_REPORT), err[-3000:]


def test_d3_adds_energy_and_virial_on_flagged_steps_and_forces_always(harness, system):
    steps = steps_of()
    rc, res, err, calls = _run(harness, system, 'd3', steps, 'd3', style_args=('9000', '1600', 'damp_bj', 'pbe'), coeff=('*', '*', 'Hf', 'O'))
    _clean(rc, err)
    _check_flagged_and_flagless(res, steps)
    assert sum(c['fn'] == 'pair_run_compute' for c in calls) == len(steps)
    assert sum(c['fn'] == 'pair_get_energy' for c in calls) == sum(bool(st[0] & 1) for st in steps)   # not even read on other steps
    for st in res['steps']:
        assert st['forces'] == [[0.25] * 3] * res['nlocal']


def test_the_driver_refuses_a_script_that_breaks_the_skin_condition(harness, system):
    struct, traj, tmp = system
    moved = [p.copy() for p in traj]
    moved[1][3, 0] += 0.6                                # skin 1.0: more than skin / 2 on a step that reuses the list
    rc, res, err, calls = _run(harness, system, 'e3gnn', steps_of(), 'skin', positions=moved)
    assert rc == 4 and 'moved more than skin / 2' in err and 'atom 4' in err, (rc, err[-2000:])
    assert len(res['steps']) == 1 and sum(c['fn'] == 'snet_md_compute' for c in calls) == 1
    ok = [p.copy() for p in traj]
    ok[3][3, 0] += 0.6                                   # the same move on a step that rebuilds is fine
    for k in (4, 5):
        ok[k][3, 0] += 0.6
    rc, res, err, calls = _run(harness, system, 'e3gnn', steps_of(), 'skin_ok', positions=ok)
    _clean(rc, err)


def test_without_a_script_the_driver_does_one_run_0_as_before(harness, system):
    exe, _ = harness
    struct, traj, tmp = system
    out = str(tmp / 'legacy.json')
    env = dict(os.environ, SNET_STUB_LOG=str(tmp / 'legacy.log'))
    r = subprocess.run([exe, 'e3gnn', struct, out, '--steps', '2', '--', '*', '*', 'stub.snet', 'Hf', 'O'], capture_output=True, text=True, env=env)
    _clean(r.returncode, r.stderr)
    res = json.load(open(out))
    assert sorted(res) == ['cutneigh', 'eatom', 'energy', 'forces', 'neigh_flags', 'nghost', 'nlocal', 'virial', 'volume']
    assert res['energy'] == 1.0 and res['virial'] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0] and res['eatom'] == [0.125] * 8
    assert res['cutneigh'] == 5.0 and res['neigh_flags'] == 1 and res['nlocal'] == 8 and res['nghost'] > 8
    calls = [json.loads(ln) for ln in open(str(tmp / 'legacy.log'))]
    assert [c['list_unchanged'] for c in calls if c['fn'] == 'snet_md_compute'] == [0, 1]
