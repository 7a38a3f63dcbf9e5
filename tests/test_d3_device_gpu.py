"""GPU: the device-resident D3 term (snet_d3_plan / snet_d3_compute_device through D3Engine.plan / compute_device, D3DeviceTerm
and SevenNetD3Calculator's d3_term='device') against the host path it stands beside.  Systems: the heterogeneous batch of
test_d3_batch_gpu (the NaCl primitive cell with thousands of images, H2O and one atom without a cell -- the box rule --, the
nine-atom triclinic cell fully periodic and with one open axis, 64 rattled Si atoms) at that file's reduced cutoffs, and the
three strained diamond cells of test_cell_relax_gpu under the mini model.

The three pair kernels are the host path's own, and the kernels around them repeat the host's IEEE operations in the host's
order with contraction off, so energy, forces and coordination numbers are compared bit for bit.  The virial is compared with
-stress V, which the host divides by V and the test multiplies back: a few ulp, inside 1e-13 of the largest entry."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cellrelax_ref as ref
from test_batch_gpu import Z
from test_cell_relax_gpu import EPS, FMAX, ORACLE_SPREAD, TRAJ_STEPS, _strained, _virial
from test_d3_batch_gpu import CUT, _engine, _many, _systems
from test_md_batch_gpu import DT, _md_args
from test_relax_gpu import D3_CUT, DEV, _all_systems, _args

pytestmark = pytest.mark.gpu

PERIODIC = [0, 2, 4]   # the fully periodic systems of _systems()


def _outside(systems):
    """the systems with every atom moved out of its cell by whole and fractional lattice vectors (molecules: by a vector)"""
    out = []
    for b, (z, pos, cell, pbc) in enumerate(systems):
        shift = np.array([1.3 + b, -2.1, 0.7]) @ cell if np.abs(cell).sum() > 0 else np.array([3.0 + b, -40.0, 0.25])
        out.append((z, np.asarray(pos, float) + shift, cell, pbc))
    return out


def _volumes(systems):
    from sevennet_amd.d3 import molecule_box
    return np.array([abs(np.linalg.det(molecule_box(s[1], s[2], s[3], *CUT)[0])) for s in systems])


def _flat(systems):
    return (np.concatenate([np.asarray(s[0]) for s in systems]), [len(s[0]) for s in systems],
            np.array([s[2] for s in systems], float), np.array([s[3] for s in systems]))


def _host_arrays(plan):
    return SimpleNamespace(**{k: getattr(plan, k).cpu().numpy().copy() for k in ('energy', 'forces', 'virial', 'cn', 'volume', 'status')})


def _assert_is_the_host_path(got, want, volumes, what=''):
    """got: _host_arrays of a device evaluation; want: D3Engine.compute_many on the same inputs"""
    from sevennet_amd.d3 import stress_to_virial
    assert got.status.tolist() == [0] * len(want), what
    a0 = 0
    for b, w in enumerate(want):
        n = len(w['forces'])
        assert got.energy[b] == w['energy'], (what, b, got.energy[b], w['energy'])
        assert np.array_equal(got.forces[a0:a0 + n], w['forces']), (what, b, 'forces')
        assert np.array_equal(got.cn[a0:a0 + n], w['cn']), (what, b, 'cn')
        vir = stress_to_virial(w['stress'], volumes[b])
        err, scale = np.abs(got.virial[b] - vir).max(), np.abs(vir).max()
        assert err <= 1e-13 * scale, (what, b, 'virial', err, scale)
        assert abs(got.volume[b] - volumes[b]) <= 1e-14 * volumes[b], (what, b, 'volume')
        a0 += n
    assert a0 == len(got.forces)


@pytest.mark.parametrize('damp', ['damp_bj', 'damp_zero'])
def test_device_evaluation_is_the_host_path_bit_for_bit(damp):
    from sevennet_amd.d3 import D3DeviceTerm
    eng = _engine(damp, 'pbe', *CUT)
    systems = _outside(_systems())
    want = _many(eng, systems)
    assert any(np.abs(w['forces']).max() > 1e-4 for w in want)
    z, n_atoms, cells, pbcs = _flat(systems)
    pos = torch.as_tensor(np.concatenate([s[1] for s in systems])).to(DEV)
    plan = eng.plan(z, n_atoms, cells, pbcs)
    got = _host_arrays(eng.compute_device(plan, pos))
    _assert_is_the_host_path(got, want, _volumes(systems), 'all six')
    _many(eng, systems[:2])   # the host path between two planned calls disturbs nothing
    again = _host_arrays(eng.compute_device(plan, pos))
    for k in ('energy', 'forces', 'virial', 'cn'):
        assert np.array_equal(getattr(again, k), getattr(got, k)), k
    # the term: a reordered subset (a re-plan), the same again (no re-plan), one system alone
    term = D3DeviceTerm(eng, z, n_atoms, cells, pbcs)
    for ids, n_plans in (([4, 0, 3, 1], 1), ([4, 0, 3, 1], 1), ([2], 2), ([5], 3)):
        sub = [systems[b] for b in ids]
        p = torch.as_tensor(np.concatenate([s[1] for s in sub])).to(DEV)
        forces, energies, virial = term(p, np.concatenate([[0], np.cumsum([len(s[0]) for s in sub])]), np.array(ids))
        assert term.n_plans == n_plans and term.provides_virial is True
        assert all(t.device == p.device and t.dtype == torch.float64 for t in (forces, energies, virial))
        assert forces.shape == (len(p), 3) and energies.shape == (len(ids),) and virial.shape == (len(ids), 6)
        assert term.status.dtype == torch.int32 and term.status.tolist() == [0] * len(ids)
        _assert_is_the_host_path(_host_arrays(term._plan), _many(eng, sub), _volumes(sub), f'systems {ids}')
    with pytest.raises(ValueError, match='replaced'):
        eng.compute_device(plan, pos)   # the engine holds one plan


_MOVING = {}


def _moving():
    """the three fully periodic systems planned at the caller's cells and evaluated at cells strained by EPS (up to 3 %, with
    shear), positions scaled with them; then again with the middle system's cell shrunk to 0.4 of its size"""
    if not _MOVING:
        eng = _engine('damp_bj', 'pbe', *CUT)
        systems = [_systems()[b] for b in PERIODIC]
        z, n_atoms, cells, pbcs = _flat(systems)
        plan = eng.plan(z, n_atoms, cells, pbcs, cells_move=True)
        D = np.eye(3) + EPS
        strained = [(zz, np.asarray(p) @ D, c @ D, pbc) for zz, p, c, pbc in systems]
        small = list(strained)
        small[1] = (strained[1][0], 0.4 * strained[1][1], 0.4 * strained[1][2], strained[1][3])
        for name, sy in (('strained', strained), ('small', small)):
            pos = torch.as_tensor(np.concatenate([s[1] for s in sy])).to(DEV)
            cd = torch.as_tensor(np.array([s[2] for s in sy]).reshape(-1, 9)).to(DEV)
            _MOVING[name] = (sy, _host_arrays(eng.compute_device(plan, pos, cd)))
        _MOVING['eng'] = eng
    return _MOVING


def test_cells_on_the_device_move_under_one_plan():
    m = _moving()
    systems, got = m['strained']
    _assert_is_the_host_path(got, _many(m['eng'], systems), _volumes(systems), 'strained')
    assert np.abs(got.virial).max() > 1e-3


def test_a_cell_beyond_the_capacity_is_flagged_and_nobody_else_notices():
    m = _moving()
    (systems, ok), (_, got) = m['strained'], m['small']
    assert got.status.tolist() == [0, 1, 0]
    sp = np.concatenate([[0], np.cumsum([len(s[0]) for s in systems])])
    assert np.isnan(got.energy[1]) and np.isnan(got.virial[1]).all() and np.isnan(got.forces[sp[1]:sp[2]]).all()
    for b in (0, 2):
        assert got.energy[b] == ok.energy[b] and np.array_equal(got.virial[b], ok.virial[b])
        assert np.array_equal(got.forces[sp[b]:sp[b + 1]], ok.forces[sp[b]:sp[b + 1]])
        assert np.array_equal(got.cn[sp[b]:sp[b + 1]], ok.cn[sp[b]:sp[b + 1]])
    assert np.isfinite(ok.forces).all() and np.isfinite(ok.virial).all()


# ------------------------------------------------------------------------------------------------ the drivers
@pytest.fixture(scope='module')
def d3calc():
    from sevennet_amd.d3 import SevenNetD3Calculator
    from sevennet_amd.shapes import mini_sevennet_0_config
    from sevennet_amd.synthetic import random_state_dict
    cfg = mini_sevennet_0_config()
    cfg = dict(cfg, _type_map={Z[s]: s for s in range(cfg['_number_of_species'])})
    return SevenNetD3Calculator((cfg, random_state_dict(cfg, seed=0)), file_type='model_instance', device=DEV, **D3_CUT)


def _assert_same_results(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y), (what, k)
        for key in x:
            assert np.array_equal(x[key], y[key], equal_nan=not isinstance(x[key], str)), (what, k, key)


def test_fixed_cell_relaxation_is_the_host_terms_bit_for_bit(d3calc):
    """three cells, the molecule and the isolated atom; the atom has no force and leaves the batch at once (repack_below 1),
    so the device term plans twice"""
    args = _args(_all_systems())
    host = d3calc.relax_many(*args, fmax=1e-4, steps=6, repack_below=1.0, d3_term='host')
    info = dict(d3calc.relax_info)
    dev = d3calc.relax_many(*args, fmax=1e-4, steps=6, repack_below=1.0, d3_term='device')
    assert d3calc.relax_info == info and info['n_repacks'] >= 1 and info['fire_launches'] == 6
    assert [r['n_steps'] for r in dev] == [6, 6, 6, 6, 0]
    _assert_same_results(dev, host, 'relax_many')
    assert not np.array_equal(dev[0]['positions'], args[1][0])


@pytest.mark.parametrize('kw', [dict(friction=0.0), dict(friction=0.02, seed=7)], ids=['nve', 'langevin'])
def test_fixed_cell_md_is_the_host_terms_bit_for_bit(d3calc, kw):
    args = _md_args(_all_systems())
    host = d3calc.md_many(*args, DT, 5, temperature=300.0, d3_term='host', **kw)
    info = dict(d3calc.md_info)
    dev = d3calc.md_many(*args, DT, 5, temperature=300.0, d3_term='device', **kw)
    assert d3calc.md_info == info == dict(n_force_calls=6, md_launches=6, system_steps_evaluated=30)
    _assert_same_results(dev, host, 'md_many')
    assert not np.array_equal(dev[0]['positions'], args[1][0]) and dev[0]['e_pot'].shape == (6,)


@pytest.fixture(scope='module')
def cell_run(d3calc):
    numbers, pos, cells, pbcs = _args(_strained())
    res = d3calc.relax_many(numbers, pos, cells, pbcs, fmax=FMAX, steps=TRAJ_STEPS, relax_cell=True, d3_term='device')
    return SimpleNamespace(numbers=numbers, pos=pos, cells=cells, pbcs=pbcs, res=res, info=dict(d3calc.relax_info))


def test_variable_cell_with_d3_follows_the_restatement(d3calc, cell_run):
    """TRAJ_STEPS steps of model + D3 on the device against cellrelax_ref.cell_fire_step driven on the host by the model's
    compute_many and D3Calculator.compute_many (forces_extra, virial_extra).  The D3 term is the same bits on both sides, so
    the two can differ by what the fp32 engine is worth over these steps only: ORACLE_SPREAD of test_cell_relax_gpu, with
    that file's margin of 10."""
    r = cell_run
    snet, d3 = d3calc.calcs
    states = [ref.cell_fire_init(p, c) for p, c in zip(r.pos, r.cells)]
    for _ in range(TRAJ_STEPS):
        at = ([s['pos'] for s in states], np.stack([s['cell'] for s in states]), r.pbcs)
        model, disp = snet.compute_many(r.numbers, *at), d3.compute_many(r.numbers, *at)
        states = [ref.cell_fire_step(s, m['forces'], _virial(m, s['cell']), FMAX, snet.cutoff / 64, forces_extra=x['forces'],
                                     virial_extra=_virial(x, s['cell']))[0] for s, m, x in zip(states, model, disp)]
    plain = snet.relax_many(r.numbers, r.pos, r.cells, r.pbcs, fmax=FMAX, steps=TRAJ_STEPS, relax_cell=True)
    assert r.info['fire_launches'] == TRAJ_STEPS and r.info['n_force_calls'] == TRAJ_STEPS + 1 and r.info['n_repacks'] == 0
    figures = []
    for b, (s, got, p) in enumerate(zip(states, r.res, plain)):
        e_pos, e_cell = np.abs(got['positions'] - s['pos']).max(), np.abs(got['cell'] - s['cell']).max()
        moved, d3_moved = np.abs(got['cell'] - r.cells[b]).max(), np.abs(got['cell'] - p['cell']).max()
        figures.append((b, e_pos, e_cell, moved, d3_moved))
        print(f'cell {b}: max |dr| {e_pos:.3e} A (bound {10 * ORACLE_SPREAD[b][0]:.1e}), max |dC| {e_cell:.3e} A (bound '
              f'{10 * ORACLE_SPREAD[b][1]:.1e}), cell moved {moved:.2e} A, D3 moved it {d3_moved:.2e} A')
    for b, e_pos, e_cell, moved, d3_moved in figures:
        s, got = states[b], r.res[b]
        assert s['n_steps'] == TRAJ_STEPS == got['n_steps'] and got['status'] == 'steps' and not got['converged']
        assert e_pos <= 10 * ORACLE_SPREAD[b][0] and e_cell <= 10 * ORACLE_SPREAD[b][1], (b, e_pos, e_cell)
        assert moved > 1e-3
        assert d3_moved > 10 * ORACLE_SPREAD[b][1], (b, d3_moved)   # the D3 virial reached the cell


def test_variable_cell_results_are_compute_many_there(d3calc, cell_run):
    """the tolerances of test_cell_relax_gpu.test_results_are_compute_many_at_the_returned_positions_and_cells"""
    r = cell_run
    many = d3calc.compute_many(r.numbers, [x['positions'] for x in r.res], np.stack([x['cell'] for x in r.res]), r.pbcs)
    old = d3calc.compute_many(r.numbers, [x['positions'] for x in r.res], r.cells, r.pbcs)   # at the caller's cells
    for b, (got, m) in enumerate(zip(r.res, many)):
        assert set(got) == set(m) | {'positions', 'converged', 'n_steps', 'cell', 'status'}
        assert abs(got['energy'] - m['energy']) <= 1e-6 * abs(m['energy']) + 1e-6, (b, got['energy'], m['energy'])
        assert np.abs(got['forces'] - m['forces']).max() <= 2e-5 * max(1.0, np.abs(m['forces']).max()), b
        assert np.abs(got['stress'] - m['stress']).max() <= 1e-5 * max(1e-3, np.abs(m['stress']).max()), b
        assert got['num_edges'] == m['num_edges']
        assert np.abs(got['stress'] - old[b]['stress']).max() > 1e-5 * max(1e-3, np.abs(m['stress']).max()), b
