"""GPU: batched FIRE relaxation -- the step kernel against its fp64 restatement (relax_ref), and the driver and the public
surfaces on a model: three rattled two-species diamond cells, the five-atom molecule and the isolated atom of the batch
tests.  Random weights have no repulsion, so fmax stays at 0.02 eV/A (at 0.002 the same model pulls two atoms of the second
cell onto each other); with the fp64 oracle driving the restatement on the CPU the three cells converge after 46 / 25 / 29
force evaluations, the molecule's forces are below fmax from the start (0.0104 eV/A) and the atom has no force at all."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import relax_ref
from helpers import oracle_model
from test_batch_gpu import Z, _calc, _systems

pytestmark = pytest.mark.gpu

FMAX = 0.02
D3_CUT = dict(vdw_cutoff=1600.0, cn_cutoff=900.0)   # the reduced cutoffs (bohr^2) of the D3 batch tests
DEV = 'cuda:0'


def _cells():
    from sevennet_amd.neighbor import diamond_cubic
    out = []
    for seed, rep, sigma in ((0, (1, 1, 1), 0.08), (1, (1, 1, 1), 0.15), (2, (2, 1, 1), 0.10)):
        pos, cell = diamond_cubic(5.431, rep, sigma, seed)
        out.append((np.random.default_rng(seed).integers(0, 2, len(pos)), pos, cell, [True] * 3))
    return out


def _all_systems():
    return _cells() + _systems(2)[4:6]   # + molecule without a cell, isolated atom


def _args(systems):
    return ([np.array(Z)[s[0]] for s in systems], [s[1] for s in systems], np.stack([s[2] for s in systems]),
            np.array([s[3] for s in systems]))


@pytest.fixture(scope='module')
def model():
    from sevennet_amd.shapes import mini_sevennet_0_config
    calc, cfg, sd = _calc(mini_sevennet_0_config())
    return SimpleNamespace(calc=calc, cfg=cfg, sd=sd, orc=oracle_model(cfg, sd))


def _oracle(model, types, pos, cell, pbc):
    from sevennet_amd.neighbor import neighbor_list
    ei, ev, _ = neighbor_list(pos, cell, pbc, model.calc.cutoff)
    out = model.orc.forward(types, ei, ev)
    return float(out['energy']), out['forces'].numpy()


# ------------------------------------------------------------------------------------------------ the kernel
class _DeviceState:
    """the per-system arrays of snet_fire_step for a list of relax_ref states"""

    def __init__(self, states):
        n = [len(s['pos']) for s in states]
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)   # noqa: E731
        self.seg_ptr = t(np.concatenate([[0], np.cumsum(n)]), torch.int32)
        self.pos = t(np.concatenate([s['pos'] for s in states]), torch.float64)
        self.vel = t(np.concatenate([s['vel'] for s in states]), torch.float64)
        self.dt = t([s['dt'] for s in states], torch.float64)
        self.alpha = t([s['alpha'] for s in states], torch.float64)
        self.n_pos = t([s['n_pos'] for s in states], torch.int32)
        self.active = t([s['active'] for s in states], torch.int32)
        self.n_steps = t([s['n_steps'] for s in states], torch.int32)
        self.fmax_sys = torch.full((len(n),), -1.0, dtype=torch.float64, device=DEV)
        self.n_active = torch.full((1,), -1, dtype=torch.int32, device=DEV)

    def step(self, forces32, fmax, extra=None, **fire):
        from sevennet_amd.relax import check_fire_params, fire_step
        f = torch.as_tensor(np.ascontiguousarray(forces32, np.float32)).to(DEV)
        x = None if extra is None else torch.as_tensor(np.ascontiguousarray(extra, np.float64)).to(DEV)
        fire_step(self.pos, self.vel, f, self.seg_ptr, self.dt, self.alpha, self.n_pos, self.active, self.n_steps, self.fmax_sys,
                  self.n_active, fmax, check_fire_params(fmax, 1, 0.5, fire), x)
        torch.cuda.synchronize()


def _compare(dev, states, what, forces64):
    """device state after one step against the restatement's next states: scalars exactly, pos / vel to 1e-11 of the array's
    largest |component| (four fp64 sums of at most 9 000 terms in another order: 9 000 x 1.1e-16 ~ 1e-12, times 10)"""
    h = lambda t: t.cpu().numpy()   # noqa: E731
    assert h(dev.n_pos).tolist() == [s['n_pos'] for s in states]
    assert h(dev.active).tolist() == [s['active'] for s in states]
    assert h(dev.n_steps).tolist() == [s['n_steps'] for s in states]
    assert h(dev.dt).tolist() == [s['dt'] for s in states]
    assert h(dev.alpha).tolist() == [s['alpha'] for s in states]
    assert int(dev.n_active.item()) == sum(s['active'] for s in states)
    for name, got in (('pos', h(dev.pos)), ('vel', h(dev.vel))):
        want = np.concatenate([s[name] for s in states])
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        assert err <= 1e-11 * scale, (name, err, scale)
    fm = h(dev.fmax_sys)
    for k, w in enumerate(what):
        if w['fm'] is not None:   # the system was active going in
            assert abs(fm[k] - w['fm']) <= 1e-14 * max(w['fm'], 1e-300), (k, fm[k], w['fm'])
            assert abs(fm[k] - np.sqrt((forces64[k] ** 2).sum(1).max())) <= 1e-14 * max(fm[k], 1e-300)


def test_kernel_follows_the_restatement_step_by_step():
    rng = np.random.default_rng(11)
    sizes, stiffness = [1, 5, 64, 3000], [40.0, 3.0, 0.6, 5.0]
    states = [relax_ref.fire_init(rng.normal(0, 0.5, (n, 3))) for n in sizes]
    seen = {'uphill': 0, 'downhill': 0, 'clipped': 0, 'frozen': 0}
    for it in range(60):
        forces = [(-k * s['pos']).astype(np.float32) for k, s in zip(stiffness, states)]   # fp32, the same bits to both sides
        dev = _DeviceState(states)
        dev.step(np.concatenate(forces), fmax=0.01)
        nxt = [relax_ref.fire_step(s, f, 0.01) for s, f in zip(states, forces)]
        states, what = [n[0] for n in nxt], [n[1] for n in nxt]
        _compare(dev, states, what, [f.astype(np.float64) for f in forces])
        for w in what:
            seen['frozen' if w['branch'] is None else w['branch']] += 1
            seen['clipped'] += bool(w['clipped'])
    # the sequence has both branches beyond the first step (every system starts uphill: v = 0), clipped moves and frozen systems
    assert seen['uphill'] > len(sizes) and seen['downhill'] > 0 and seen['clipped'] > 0 and seen['frozen'] > 0, seen


def test_kernel_adds_the_second_force_array_in_fp64():
    rng = np.random.default_rng(5)
    states = [relax_ref.fire_init(rng.normal(0, 0.5, (n, 3))) for n in (7, 300)]
    for it in range(12):
        f32 = [(-2.0 * s['pos']).astype(np.float32) for s in states]
        f64 = [1e-3 * np.sin(3.0 * s['pos']) for s in states]
        dev = _DeviceState(states)
        dev.step(np.concatenate(f32), fmax=0.01, extra=np.concatenate(f64))
        total = [a.astype(np.float64) + b for a, b in zip(f32, f64)]
        nxt = [relax_ref.fire_step(s, f, 0.01) for s, f in zip(states, total)]
        states, what = [n[0] for n in nxt], [n[1] for n in nxt]
        _compare(dev, states, what, total)


def test_frozen_means_frozen():
    """an inactive system, and one whose forces are already below fmax, keep pos and vel bit for bit; the second is switched
    off without a step counted; the third moves"""
    rng = np.random.default_rng(3)
    states = [relax_ref.fire_init(rng.normal(0, 1.0, (n, 3))) for n in (40, 300, 9)]
    for s in states:
        s['vel'] = rng.normal(0, 0.1, s['pos'].shape)
        s['n_steps'], s['n_pos'], s['dt'], s['alpha'] = 4, 2, 0.07, 0.09
    states[0]['active'] = 0
    forces = [rng.normal(0, 5.0, (40, 3)), rng.normal(0, 1e-3, (300, 3)), rng.normal(0, 1.0, (9, 3))]
    dev = _DeviceState(states)
    pos0, vel0 = dev.pos.clone(), dev.vel.clone()
    dev.step(np.concatenate(forces), fmax=0.05)
    assert torch.equal(dev.pos[:340], pos0[:340]) and torch.equal(dev.vel[:340], vel0[:340])
    assert not torch.equal(dev.pos[340:], pos0[340:])
    assert dev.active.tolist() == [0, 0, 1] and dev.n_steps.tolist() == [4, 4, 5] and int(dev.n_active.item()) == 1
    assert dev.dt.tolist()[:2] == [0.07, 0.07] and dev.alpha.tolist()[:2] == [0.09, 0.09] and dev.n_pos.tolist()[:2] == [2, 2]
    assert dev.fmax_sys[0].item() == -1.0 and 0 < dev.fmax_sys[1].item() < 0.05   # untouched / reported


# ------------------------------------------------------------------------------------------------ the driver on a model
def _check_relaxed(model, systems, res, initial):
    """the assertions on a finished relaxation, per system: converged; the fp64 oracle's largest atomic force at the returned
    positions below fmax + 1e-4 eV/A (the project's force-parity bar); energy and forces equal to calc.compute there within
    the batch-vs-single tolerances of test_batch_equals_single_structure_calls; energy below the initial one for every system
    that moved (the molecule and the atom are below fmax where they start: n_steps = 0, nothing to lower)"""
    calc = model.calc
    for b, (types, pos, cell, pbc) in enumerate(systems):
        r = res[b]
        assert r['converged'], b
        assert r['positions'].shape == pos.shape and r['positions'].dtype == np.float64
        e_orc, f_orc = _oracle(model, types, r['positions'], cell, pbc)
        fm_orc = np.sqrt((f_orc ** 2).sum(1).max())
        print(f'system {b}: n_steps {r["n_steps"]}, oracle max|F| {fm_orc:.5f} eV/A, E {initial[b]["energy"]:.6f} -> {r["energy"]:.6f}')
        assert fm_orc < FMAX + 1e-4, (b, fm_orc)
        one = calc.compute(np.array(Z)[types], r['positions'], cell, pbc)
        assert abs(r['energy'] - one['energy']) <= 1e-6 * abs(one['energy']) + 1e-6, (b, r['energy'], one['energy'])
        assert np.abs(r['forces'] - one['forces']).max() <= 2e-5 * max(1.0, np.abs(one['forces']).max()), b
        if r['n_steps'] > 0:
            assert r['energy'] < initial[b]['energy'], (b, r['energy'], initial[b]['energy'])
        else:
            assert np.array_equal(r['positions'], pos)
    atom = res[-1]
    assert atom['n_steps'] == 0 and np.array_equal(atom['positions'], systems[-1][1])


def test_relax_many_end_to_end(model):
    systems = _all_systems()
    initial = model.calc.compute_many(*_args(systems))
    res = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=200)
    _check_relaxed(model, systems, res, initial)
    info = model.calc.relax_info
    steps = [r['n_steps'] for r in res]
    assert steps[3:] == [0, 0] and all(10 < s < 200 for s in steps[:3]), steps
    # one launch per loop iteration: the slowest system is found converged by the launch after its last move
    assert info['fire_launches'] == max(steps) + 1 and info['n_force_calls'] == info['fire_launches'] + 1
    for k in ('free_energy', 'energy', 'energies', 'forces', 'stress', 'num_edges', 'positions', 'converged', 'n_steps'):
        assert k in res[0]


def test_two_runs_are_identical(model):
    systems = _all_systems()
    a = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=200)
    b = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=200)
    for x, y in zip(a, b):
        assert np.array_equal(x['positions'], y['positions']) and x['energy'] == y['energy'] and x['n_steps'] == y['n_steps']
        assert np.array_equal(x['forces'], y['forces'])


def test_first_steps_follow_the_oracle_trajectory(model):
    """positions after 10 steps against the restatement driven by the fp64 oracle's forces: within 1e-4 (sum_k dt_k)^2 A, what
    a force error at the 1e-4 eV/A bar can displace over those steps; needs the same P > 0 decisions, which are nowhere near a
    tie (cosine of F and v at least 0.5 from the second step on; 0.999 when this was written)"""
    systems = _cells()
    res = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=10)
    for b, (types, pos, cell, pbc) in enumerate(systems):
        s, log, dts = relax_ref.fire_relax(pos, lambda p: _oracle(model, types, p, cell, pbc)[1], FMAX, 10)
        assert len(dts) == 10 and s['n_steps'] == 10 and res[b]['n_steps'] == 10 and not res[b]['converged']
        assert min(w['cos'] for w in log[1:]) > 0.5, [w['cos'] for w in log]
        tol = 1e-4 * sum(dts) ** 2
        err = np.abs(res[b]['positions'] - s['pos']).max()
        print(f'cell {b}: max |dr| {err:.3e} A (bound {tol:.3e}), min cos {min(w["cos"] for w in log[1:]):.4f}')
        assert err <= tol, (b, err, tol)


def test_repacking(model):
    systems = _all_systems()
    B = len(systems)
    initial = model.calc.compute_many(*_args(systems))
    res = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=200, repack_below=1.0)
    info = dict(model.calc.relax_info)
    assert info['n_repacks'] >= 1
    assert info['system_steps_evaluated'] < B * max(r['n_steps'] for r in res)
    _check_relaxed(model, systems, res, initial)   # (per system and by index: the caller's order)
    for r, s in zip(res, systems):
        assert r['positions'].shape == s[1].shape and np.abs(r['positions'] - s[1]).max() < 1.0
    res0 = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=200, repack_below=0)
    info0 = model.calc.relax_info
    assert info0['n_repacks'] == 0 and info0['system_steps_evaluated'] == B * info0['fire_launches']
    assert info0['n_force_calls'] == info0['fire_launches'] + 1
    _check_relaxed(model, systems, res0, initial)


def test_step_cap(model):
    systems = _all_systems()
    res = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=3)
    for r in res[:3]:
        assert r['converged'] is False and r['n_steps'] == 3
        assert np.isfinite(r['energy']) and np.isfinite(r['forces']).all() and np.isfinite(r['positions']).all()
        assert np.isfinite(r['stress']).all()
    assert [r['converged'] for r in res[3:]] == [True, True] and [r['n_steps'] for r in res[3:]] == [0, 0]
    assert model.calc.relax_info['fire_launches'] == 3
    none = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=0)   # no step at all: the evaluation only
    assert all(not r['converged'] and r['n_steps'] == 0 for r in none) and model.calc.relax_info['fire_launches'] == 0
    assert all(np.array_equal(r['positions'], s[1]) for r, s in zip(none, systems))


def test_one_launch_per_step_whatever_the_batch(model):
    """fire_launches equals the loop iterations -- the slowest system's moves plus the launch that finds it converged --
    for one system and for a batch of 15"""
    cells = _cells()
    one = model.calc.relax_many(*_args(cells[:1]), fmax=FMAX, steps=200, repack_below=0)
    assert model.calc.relax_info['fire_launches'] == one[0]['n_steps'] + 1
    many = _all_systems() * 3
    res = model.calc.relax_many(*_args(many), fmax=FMAX, steps=200, repack_below=0)
    info = model.calc.relax_info
    assert info['fire_launches'] == max(r['n_steps'] for r in res) + 1
    assert info['system_steps_evaluated'] == len(many) * info['fire_launches']


def test_d3_sum_relaxes(model):
    from sevennet_amd.d3 import SevenNetD3Calculator
    calc = SevenNetD3Calculator((model.cfg, model.sd), file_type='model_instance', device=DEV, **D3_CUT)
    systems = _cells()
    res = calc.relax_many(*_args(systems), fmax=FMAX, steps=200)
    assert calc.relax_info['fire_launches'] == max(r['n_steps'] for r in res) + 1
    for b, (types, pos, cell, pbc) in enumerate(systems):
        r = res[b]
        assert r['converged'], b
        one = calc.compute(np.array(Z)[types], r['positions'], cell, pbc)
        fm = np.sqrt((one['forces'] ** 2).sum(1).max())
        print(f'cell {b} with D3: n_steps {r["n_steps"]}, max|F| {fm:.5f} eV/A')
        assert fm < FMAX + 2e-5 * max(1.0, np.abs(one['forces']).max()), (b, fm)
        assert set(r) == set(one) | {'positions', 'converged', 'n_steps'}
        assert np.abs(r['forces'] - one['forces']).max() <= 2e-5 * max(1.0, np.abs(one['forces']).max())


class _Atoms:
    """what relax_many_atoms reads from and writes to an ASE Atoms"""

    def __init__(self, z, pos, cell, pbc):
        self.z, self.pos, self.cell, self.pbc = z, np.array(pos, float), cell, pbc

    def get_atomic_numbers(self):
        return np.asarray(self.z)

    def get_positions(self):
        return self.pos.copy()

    def get_cell(self):
        return np.asarray(self.cell, float)

    def get_pbc(self):
        return np.asarray(self.pbc, bool)

    def set_positions(self, pos):
        self.pos = np.array(pos, float)


def test_surfaces(model):
    from sevennet_amd.d3 import SevenNetD3Calculator
    systems = _all_systems()
    atoms = [_Atoms(np.array(Z)[s[0]], s[1], s[2], s[3]) for s in systems]
    res = model.calc.relax_many_atoms(atoms, fmax=FMAX, steps=200)
    ref = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=200)
    one = model.calc.compute(*[a[0] for a in _args(systems[:1])])
    for a, r, q, s in zip(atoms, res, ref, systems):
        assert np.array_equal(a.get_positions(), r['positions']) and np.array_equal(r['positions'], q['positions'])
        assert set(r) == set(one) | {'positions', 'converged', 'n_steps'}
    assert not np.array_equal(atoms[0].get_positions(), systems[0][1])
    d3 = SevenNetD3Calculator((model.cfg, model.sd), file_type='model_instance', device=DEV, **D3_CUT)
    atoms = [_Atoms(np.array(Z)[s[0]], s[1], s[2], s[3]) for s in systems[:2]]
    res = d3.relax_many_atoms(atoms, fmax=FMAX, steps=5)
    assert all(np.array_equal(a.get_positions(), r['positions']) and r['n_steps'] == 5 for a, r in zip(atoms, res))
    with pytest.raises(ValueError, match='Model do not know atomic number: 79'):
        model.calc.relax_many([[79]], [np.zeros((1, 3))], np.zeros((1, 3, 3)), [False] * 3)
