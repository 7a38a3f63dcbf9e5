"""CPU: batched MD -- the Philox generator of the restatement (md_ref) against Random123's published vectors, the restated
BAOAB rule on a harmonic well, and md_batch's input validation before any device work.  The driver itself cannot run on CPU
tensors (its neighbor build, engine call and step are HIP kernels, and there is no CPU path): the loop is covered on the GPU
(test_md_batch_gpu.py)."""
from types import SimpleNamespace

import numpy as np
import pytest

import md_ref


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize('counter, key, want', [
    ('00000000 00000000 00000000 00000000', '00000000 00000000', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff', '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0', 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_philox_known_answers(counter, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds"""
    words = lambda s: [int(w, 16) for w in s.split()]   # noqa: E731
    got = md_ref.philox4x32(np.array(words(counter)), np.array(words(key)))
    assert got.dtype == np.uint32 and got.tolist() == words(want)


def test_philox_is_vectorised_and_the_normals_are_the_stated_ones():
    ctr = np.array([[0, 0, 0, 0], [3, 7, 11, 1], [0xffffffff] * 4])
    all_at_once = md_ref.philox4x32(ctr, [5, 9])
    assert all(np.array_equal(all_at_once[i], md_ref.philox4x32(ctr[i], [5, 9])) for i in range(3))
    seed = (0x1234 << 32) | 0xabcd
    xi = md_ref.normals(seed, sys_id=7, n=5, step=11, stream_tag=1)
    w = md_ref.philox4x32([3, 7, 11, 1], [0xabcd, 0x1234]).astype(np.float64)
    u = (w + 0.5) / 2.0 ** 32
    assert ((u > 0) & (u < 1)).all()
    r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
    assert np.array_equal(xi[3], [r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]), r1 * np.cos(2 * np.pi * u[3])])
    # another system, step, stream or seed: other numbers
    for other in (md_ref.normals(seed, 8, 5, 11, 1), md_ref.normals(seed, 7, 5, 12, 1), md_ref.normals(seed, 7, 5, 11, 0),
                  md_ref.normals(seed + 1, 7, 5, 11, 1)):
        assert not np.any(other == xi)
    big = md_ref.normals(3, 0, 20000, 0, 0).ravel()
    M = big.size
    assert abs(big.mean()) <= 5 / np.sqrt(M) and abs(big.var() - 1) <= 5 * np.sqrt(2 / M)


# ------------------------------------------------------------------------------------------------ the rule on a harmonic well
K_WELL = 2.0          # eV / A^2
MASS = np.array([1.008, 15.999, 28.0855, 15.999])


def _well(pos):
    return 0.5 * K_WELL * float((pos ** 2).sum()), -K_WELL * pos


def _x0v0():
    rng = np.random.default_rng(0)
    return rng.normal(0, 0.3, (4, 3)), rng.normal(0, 0.01, (4, 3))


def test_nve_energy_error_scales_as_dt_squared():
    """the lightest atom's period is 2 pi sqrt(m / (k ACC)) = 45 fs; 40 fs at dt = 0.5 and 0.25 fs"""
    x0, v0 = _x0v0()
    err = []
    for dt in (0.5, 0.25):
        r = md_ref.md_run(x0, _well, MASS, dt, int(round(40.0 / dt)), vel=v0)
        e = r['e_pot'] + r['e_kin']
        err.append(np.abs(e - e[0]).max())
        assert r['step'] == int(round(40.0 / dt)) and len(e) == r['step'] + 1
    assert err[0] > 1e-6 and 3.5 < err[0] / err[1] < 4.5, err


def test_c1_one_c2_zero_is_velocity_verlet():
    x0, v0 = _x0v0()
    dt, steps, m = 0.4, 30, MASS[:, None]
    x, v = x0.copy(), v0.copy()
    f = _well(x)[1]
    for _ in range(steps):   # the loop of tools/md_loop.run_md
        v = v + 0.5 * dt * md_ref.ACC * f / m
        x = x + dt * v
        f = _well(x)[1]
        v = v + 0.5 * dt * md_ref.ACC * f / m
    assert md_ref.langevin_coefficients(0.0, dt) == (1.0, 0.0)
    r = md_ref.md_run(x0, _well, MASS, dt, steps, vel=v0)
    assert np.abs(r['pos'] - x).max() <= 1e-13 * np.abs(x).max() and np.abs(r['vel'] - v).max() <= 1e-13 * np.abs(v).max()
    assert abs(r['e_kin'][-1] - md_ref.kinetic_energy(MASS, v)) <= 1e-13 * r['e_kin'][-1]
    assert np.array_equal(r['traj'][0], x0) and np.array_equal(r['traj'][-1], r['pos'])
    # the single steps: phase 0 moves nothing, FINISH alone leaves the positions and the step counter
    s = md_ref.md_init(x0, v0, step=4)
    s0, ek = md_ref.md_step(s, f, MASS, 0.0, dt, 1.0, 0.0, 0, 0, 0)
    assert np.array_equal(s0['pos'], x0) and np.array_equal(s0['vel'], v0) and s0['step'] == 4 and ek == md_ref.kinetic_energy(MASS, v0)
    s1, _ = md_ref.md_step(s, f, MASS, 0.0, dt, 1.0, 0.0, 0, 0, md_ref.FINISH)
    assert np.array_equal(s1['pos'], x0) and s1['step'] == 4 and not np.array_equal(s1['vel'], v0)
    assert np.array_equal(s['pos'], x0) and np.array_equal(s['vel'], v0)   # the input is not modified


def test_langevin_step_uses_the_step_indexed_noise():
    """F = 0, v = 0, c1 = 0, c2 = 1: after START the velocity is sqrt(kT ACC / m) xi of the state's step, and x has moved half
    a step with it"""
    x0 = np.zeros((4, 3))
    kT = 0.025
    s, ek = md_ref.md_step(md_ref.md_init(x0, step=9), np.zeros((4, 3)), MASS, kT, 0.5, 0.0, 1.0, 42, 3, md_ref.START)
    xi = md_ref.normals(42, 3, 4, 9, md_ref.STREAM_THERMOSTAT)
    assert ek == 0.0 and s['step'] == 10
    assert np.array_equal(s['vel'], np.sqrt(kT * md_ref.ACC / MASS[:, None]) * xi) and np.array_equal(s['pos'], 0.25 * s['vel'])


def test_init_velocities_momentum_and_temperature():
    rng = np.random.default_rng(1)
    for n in (2, 5, 300):
        m = rng.choice([1.008, 15.999, 28.0855], n)
        kT = md_ref.KB * 300.0
        v = md_ref.init_velocities(m, kT, seed=5, sys_id=2)
        p = (m[:, None] * v).sum(0)
        assert np.abs(p).max() <= 1e-12 * (m[:, None] * np.abs(v)).sum()
        assert abs(md_ref.kinetic_energy(m, v) - 0.5 * (3 * n - 3) * kT) <= 1e-12 * 0.5 * (3 * n - 3) * kT
        raw = md_ref.init_velocities(m, kT, seed=5, sys_id=2, remove_com=False)
        assert np.array_equal(raw, np.sqrt(kT * md_ref.ACC / m[:, None]) * md_ref.normals(5, 2, n, 0, md_ref.STREAM_INIT))
    assert np.array_equal(md_ref.init_velocities([12.0], 0.02, 5, 0), np.zeros((1, 3)))
    assert md_ref.init_velocities([12.0], 0.02, 5, 0, remove_com=False).any()


# ------------------------------------------------------------------------------------------------ validation
class _NoDeviceEngine:
    """stands for a HipForceEngine in calls that must fail before they reach it: any use beyond spec.num_species is an error"""
    spec = SimpleNamespace(num_species=2)

    def __getattr__(self, name):
        raise AssertionError(f'the engine was touched ({name}) before the input was validated')


def _two_systems():
    types = [np.array([0, 1]), np.array([1])]
    pos = [np.array([[0.0, 0, 0], [1.2, 0, 0]]), np.array([[0.0, 0, 0]])]
    masses = [np.array([28.0855, 15.999]), np.array([15.999])]
    cells = np.stack([np.eye(3) * 6.0, np.zeros((3, 3))])
    pbcs = np.array([[True] * 3, [False] * 3])
    return types, pos, masses, cells, pbcs


def _md(monkeypatch, **kw):
    import torch
    from sevennet_amd.md import md_batch

    def touched(*a, **k):
        raise AssertionError('torch.cuda was touched before the input was validated')
    for name in ('device', 'current_stream', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, touched)
    types, pos, masses, cells, pbcs = _two_systems()
    args = dict(types=types, positions=pos, masses=masses, cells=cells, pbcs=pbcs, cutoff=5.0, dt=1.0, steps=3, temperature=300.0)
    args.update(kw)
    return md_batch(_NoDeviceEngine(), args.pop('types'), args.pop('positions'), args.pop('masses'), args.pop('cells'),
                    args.pop('pbcs'), **args)


_V = [np.zeros((2, 3)), np.zeros((1, 3))]


@pytest.mark.parametrize('kw, match', [
    (dict(dt=0.0), 'dt'),
    (dict(dt=-1.0), 'dt'),
    (dict(dt=float('nan')), 'dt'),
    (dict(steps=-1), 'steps'),
    (dict(steps=2.5), 'steps'),
    (dict(friction=-0.1), 'friction'),
    (dict(friction=None), 'friction'),
    (dict(friction='0.01'), 'friction'),
    (dict(friction=1e-17), 'below fp64 resolution'),
    (dict(seed=1.5), 'seed'),
    (dict(temperature=-1.0), 'system 0: temperature'),
    (dict(temperature=[300.0, -5.0]), 'system 1: temperature'),
    (dict(temperature=[300.0, 300.0, 300.0]), 'temperature of shape'),
    (dict(masses=[np.array([28.0855, 0.0]), np.array([15.999])]), 'system 0: mass'),
    (dict(masses=[np.array([28.0855, 15.999]), np.array([-1.0])]), 'system 1: mass'),
    (dict(masses=[np.array([28.0855, 15.999]), np.array([np.inf])]), 'system 1: mass'),
    (dict(masses=[np.array([28.0855, np.nan]), np.array([15.999])]), 'system 0: mass'),
    (dict(masses=[np.array([28.0855]), np.array([15.999])]), 'system 0: masses of shape'),
    (dict(masses=[np.array([28.0855, 15.999])]), 'masses'),
    (dict(masses=np.ones(4)), 'masses of shape'),
    (dict(velocities=[np.zeros((2, 3)), np.zeros((2, 3))]), 'system 1: velocities of shape'),
    (dict(velocities=[np.zeros((2, 2)), np.zeros((1, 3))]), 'system 0: velocities of shape'),
    (dict(velocities=np.zeros((4, 3))), 'velocities of shape'),
    (dict(velocities=[np.zeros((2, 3)), np.full((1, 3), np.nan)]), 'system 1: non-finite velocity'),
    (dict(log_every=0), 'log_every'),
    (dict(log_every=1.5), 'log_every'),
    (dict(traj_every=-1), 'traj_every'),
    (dict(traj_every=0.5), 'traj_every'),
    (dict(temperature=None), 'neither velocities nor temperature'),
    (dict(temperature=None, velocities=_V, friction=0.01), 'friction'),
    (dict(seed=-1), 'seed'),
    (dict(system_ids=[0]), 'system_ids'),
    (dict(cutoff=0.0), 'cutoff'),
    (dict(types=[np.array([0, 1]), np.array([2])]), 'system 1: unknown species index 2'),
])
def test_bad_input_raises_before_any_device_work(monkeypatch, kw, match):
    with pytest.raises(ValueError, match=match):
        _md(monkeypatch, **kw)


def test_batch_forces_is_constructed_without_any_device_work(monkeypatch):
    """BatchForces on the engine that may not be touched, with torch.cuda.device / current_stream / synchronize raising"""
    import torch
    from sevennet_amd.batch import BatchForces, validate_batch_inputs

    def touched(*a, **k):
        raise AssertionError('torch.cuda was touched by the constructor')
    for name in ('device', 'current_stream', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, touched)
    types, pos, _, cells, pbcs = _two_systems()
    ty, _, n_at, cells, pbcs = validate_batch_inputs(types, pos, cells, pbcs, 5.0, 2)
    forces = BatchForces(_NoDeviceEngine(), ty, n_at, cells, pbcs, 5.0, extra=lambda *a: None)
    assert (forces.n_force_calls, forces.system_steps_evaluated) == (0, 0)


def test_validated_inputs_are_copies_in_the_stated_units():
    from sevennet_amd.md import ACC, KB, langevin_coefficients, validate_md_inputs
    assert (ACC, KB) == (md_ref.ACC, md_ref.KB)
    n_at = np.array([2, 1])
    masses = [np.array([28.0855, 15.999]), np.array([15.999])]
    mass, vel, kT, ids = validate_md_inputs(masses, n_at, 1.0, 3, [300.0, 0.0], 0.01, None, 7, 1, 0)
    assert mass.tolist() == [28.0855, 15.999, 15.999] and vel is None and kT.tolist() == [KB * 300.0, 0.0] and ids.tolist() == [0, 1]
    flat_v = np.arange(9.0).reshape(3, 3)
    mass, vel, kT, ids = validate_md_inputs(np.array([1.0, 2.0, 3.0]), n_at, 1.0, 0, None, 0.0, flat_v, 0, 1, 0, system_ids=[5, 2])
    assert np.array_equal(vel, flat_v) and vel is not flat_v and kT.tolist() == [0.0, 0.0] and ids.tolist() == [5, 2]
    assert ids.dtype == np.int32
    assert langevin_coefficients(0.0, 2.0) == (1.0, 0.0) == md_ref.langevin_coefficients(0.0, 2.0)
    assert langevin_coefficients(0.1, 0.5) == md_ref.langevin_coefficients(0.1, 0.5)   # the same bits on both sides


def test_surfaces_exist():
    from sevennet_amd import _lib
    from sevennet_amd.calculator import SevenNetCalculator
    from sevennet_amd.d3 import SevenNetD3Calculator
    for cls in (SevenNetCalculator, SevenNetD3Calculator):
        assert callable(cls.md_many) and callable(cls.md_many_atoms)
    assert len(_lib.SIGNATURES['snet_mdb_step'][1]) == 18 and len(_lib.SIGNATURES['snet_mdb_init_velocities'][1]) == 10
    lib = _lib.load()
    assert hasattr(lib, 'snet_mdb_step') and hasattr(lib, 'snet_mdb_init_velocities')


def test_ase_objects_are_refused_without_explicit_velocities():
    """their velocity unit is A / (10.18 fs): read as A/fs it would be wrong tenfold without a sign of it"""
    from sevennet_amd.atoms import atoms_velocities

    class Duck:
        def __init__(self, v):
            self.v = v

        def get_velocities(self):
            return self.v
    v = np.ones((2, 3))
    assert np.array_equal(atoms_velocities([Duck(v), Duck(2 * v)], dict(seed=1))['velocities'][1], 2 * v)
    assert 'velocities' not in atoms_velocities([Duck(v), Duck(None)], {}) and 'velocities' not in atoms_velocities([object()], {})
    FromAse = type('Atoms', (Duck,), {'__module__': 'ase.atoms'})
    with pytest.raises(ValueError, match='system 1 is an ase object'):
        atoms_velocities([Duck(v), FromAse(v)], {})
    given = dict(velocities=[v, v])
    assert atoms_velocities([Duck(v), FromAse(v)], given) is given
