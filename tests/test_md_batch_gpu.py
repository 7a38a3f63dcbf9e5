"""GPU: batched MD -- the step kernel and the velocity draw against their fp64 restatement (md_ref), and the driver and the
public surfaces on a model: the three rattled two-species diamond cells of the relax tests, the five-atom molecule and the
isolated atom.  Kernel tests use synthetic fp32 forces (the same bits on both sides) and systems of 1, 5, 64 and 3000 atoms:
a single lane, part of a wave, a quarter workgroup and twelve strides of the loop."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import md_ref
from helpers import oracle_model
from test_batch_gpu import Z, _calc
from test_relax_gpu import D3_CUT, DEV, _all_systems, _args, _cells, _oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 64, 3000]
MASS_OF = np.array([28.0855, 15.999])   # amu, of species 0 / 1 (Z = 14, 8)
DT, STEPS = 1.0, 12


def _masses(rng, sizes=SIZES):
    return [rng.choice([1.008, 15.999, 28.0855], n) for n in sizes]


def _up(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _h(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the kernel
class _DeviceState:
    """the arrays of snet_mdb_step for a list of md_ref states"""

    def __init__(self, states, masses, kT, sys_id=None):
        n = [len(s['pos']) for s in states]
        self.n = n
        self.seg_ptr = _up(np.concatenate([[0], np.cumsum(n)]), torch.int32)
        self.pos = _up(np.concatenate([s['pos'] for s in states]), torch.float64)
        self.vel = _up(np.concatenate([s['vel'] for s in states]), torch.float64)
        self.mass = _up(np.concatenate(masses), torch.float64)
        self.kT = _up(kT, torch.float64)
        self.sys_id = _up(np.arange(len(n)) if sys_id is None else sys_id, torch.int32)
        self.step_index = _up([s['step'] for s in states], torch.int32)
        self.e_kin = torch.full((len(n),), -1.0, dtype=torch.float64, device=DEV)

    def step(self, forces32, dt, c1, c2, seed, phase, extra=None):
        from sevennet_amd.md import md_step
        f = _up(forces32, torch.float32)
        x = None if extra is None else _up(extra, torch.float64)
        md_step(self.pos, self.vel, f, self.mass, self.seg_ptr, self.sys_id, self.kT, self.step_index, self.e_kin, dt, c1, c2, seed,
                phase, x)
        torch.cuda.synchronize()


def test_noise_is_the_stated_noise():
    """v = 0, F = 0, c1 = 0, c2 = 1, unit masses and kT = 1 / ACC: after START `vel` is xi (times sqrt(kT ACC / m) = 1 to an ulp)
    and x = x0 + (dt/2) xi.  Against md_ref's normals within 1e-14 absolute: a few ulp of fp64 log / sin / cos on |xi| <= 7."""
    seed, steps0 = (0x9abcdef0 << 32) | 0x12345678, [0, 3, 17, 1000]
    states = [md_ref.md_init(np.zeros((n, 3)), step=k) for n, k in zip(SIZES, steps0)]
    dev = _DeviceState(states, [np.ones(n) for n in SIZES], np.full(4, 1.0 / md_ref.ACC))
    dev.step(np.zeros((sum(SIZES), 3)), 0.5, 0.0, 1.0, seed, md_ref.START)
    want = np.concatenate([md_ref.normals(seed, b, n, k, md_ref.STREAM_THERMOSTAT) for b, (n, k) in enumerate(zip(SIZES, steps0))])
    got = _h(dev.vel)
    err = np.abs(got - want).max()
    print(f'noise: max |xi - restatement| {err:.2e}, max |xi| {np.abs(want).max():.2f}')
    assert err <= 1e-14
    assert np.abs(_h(dev.pos) - 0.25 * got).max() <= 1e-15
    assert _h(dev.step_index).tolist() == [k + 1 for k in steps0] and _h(dev.e_kin).tolist() == [0.0] * 4
    M = got.size
    assert M == 3 * 3070
    assert abs(got.mean()) <= 5 / np.sqrt(M) and abs(got.var() - 1) <= 5 * np.sqrt(2 / M), (got.mean(), got.var())


@pytest.mark.parametrize('gamma_dt', [0.0, 0.05], ids=['nve', 'langevin'])
def test_kernel_follows_the_restatement_step_by_step(gamma_dt):
    """40 steps in 41 launches, phase 2, 3, ..., 3, 1, the device state rebuilt from the restatement's each time: step_index exactly, pos / vel
    to 1e-11 of the array's largest |component|, e_kin to 1e-11 relative (one fp64 sum of at most 9 000 terms in another order:
    9 000 x 1.1e-16 ~ 1e-12, times 10).  The Langevin sequence also carries a second, fp64 force array."""
    rng = np.random.default_rng(11)
    stiffness, dt, seed = [40.0, 3.0, 0.6, 5.0], 0.5, 77
    masses = _masses(rng)
    kT = md_ref.KB * np.array([100.0, 300.0, 600.0, 1000.0])
    c1, c2 = md_ref.langevin_coefficients(gamma_dt / dt, dt)
    assert (c2 == 0.0) == (gamma_dt == 0.0)
    states = [md_ref.md_init(rng.normal(0, 0.5, (n, 3)), rng.normal(0, 0.01, (n, 3))) for n in SIZES]
    n_launch = 41
    for it in range(n_launch):
        phase = md_ref.START if it == 0 else (md_ref.FINISH if it == n_launch - 1 else md_ref.FINISH | md_ref.START)
        f32 = [(-k * s['pos']).astype(np.float32) for k, s in zip(stiffness, states)]   # fp32, the same bits to both sides
        f64 = [1e-3 * np.sin(3.0 * s['pos']) if gamma_dt else None for s in states]
        dev = _DeviceState(states, masses, kT)
        dev.step(np.concatenate(f32), dt, c1, c2, seed, phase, np.concatenate(f64) if gamma_dt else None)
        total = [a.astype(np.float64) + (b if gamma_dt else 0.0) for a, b in zip(f32, f64)]
        nxt = [md_ref.md_step(s, f, m, t, dt, c1, c2, seed, b, phase) for b, (s, f, m, t) in enumerate(zip(states, total, masses, kT))]
        states, e_kin = [x[0] for x in nxt], np.array([x[1] for x in nxt])
        assert _h(dev.step_index).tolist() == [s['step'] for s in states]
        for name, got in (('pos', _h(dev.pos)), ('vel', _h(dev.vel))):
            want = np.concatenate([s[name] for s in states])
            err, scale = np.abs(got - want).max(), np.abs(want).max()
            assert err <= 1e-11 * scale, (it, name, err, scale)
        assert (np.abs(_h(dev.e_kin) - e_kin) <= 1e-11 * e_kin).all(), (it, _h(dev.e_kin), e_kin)
    assert [s['step'] for s in states] == [n_launch - 1] * 4


def test_phases():
    """phase 0 writes e_kin and nothing else; phase 1 (FINISH) leaves positions and step counters; without a thermostat (c2 = 0)
    the seed is not read"""
    rng = np.random.default_rng(3)
    masses = _masses(rng)
    kT = np.full(4, md_ref.KB * 300.0)
    states = [md_ref.md_init(rng.normal(0, 0.5, (n, 3)), rng.normal(0, 0.01, (n, 3)), step=5) for n in SIZES]
    forces = rng.normal(0, 1.0, (sum(SIZES), 3))
    dev = _DeviceState(states, masses, kT)
    pos0, vel0 = dev.pos.clone(), dev.vel.clone()
    dev.step(forces, 0.5, 1.0, 0.0, 1, 0)
    assert torch.equal(dev.pos, pos0) and torch.equal(dev.vel, vel0) and _h(dev.step_index).tolist() == [5] * 4
    want = np.array([md_ref.kinetic_energy(m, s['vel']) for m, s in zip(masses, states)])
    assert (np.abs(_h(dev.e_kin) - want) <= 1e-11 * want).all()
    dev.step(forces, 0.5, 1.0, 0.0, 1, md_ref.FINISH)
    assert torch.equal(dev.pos, pos0) and not torch.equal(dev.vel, vel0) and _h(dev.step_index).tolist() == [5] * 4
    a, b = _DeviceState(states, masses, kT), _DeviceState(states, masses, kT)
    a.step(forces, 0.5, 1.0, 0.0, 1, 3)
    b.step(forces, 0.5, 1.0, 0.0, 2 ** 63 + 12345, 3)
    assert torch.equal(a.pos, b.pos) and torch.equal(a.vel, b.vel) and torch.equal(a.e_kin, b.e_kin)
    assert not torch.equal(a.pos, pos0) and _h(a.step_index).tolist() == [6] * 4
    c = _DeviceState(states, masses, kT)
    c.step(forces, 0.5, 0.9, float(np.sqrt(1 - 0.81)), 1, 3)   # (with a thermostat the same call does read it)
    d = _DeviceState(states, masses, kT)
    d.step(forces, 0.5, 0.9, float(np.sqrt(1 - 0.81)), 2, 3)
    assert not torch.equal(c.vel, d.vel)


def test_entry_points_check_their_ranges():
    """out-of-range scalars and a missing array are refused (rc 2, nothing launched); on real device tensors, so that a check
    that went missing would give a wrong result and not a fault"""
    import ctypes as C
    from sevennet_amd import _lib
    from sevennet_amd.md import init_velocities
    lib = _lib.load()
    rng = np.random.default_rng(2)
    dev = _DeviceState([md_ref.md_init(rng.normal(0, 0.5, (n, 3)), rng.normal(0, 0.01, (n, 3))) for n in (5, 64)],
                       _masses(rng, (5, 64)), np.full(2, 0.02))
    f = _up(np.zeros((69, 3)), torch.float32)
    pos0, vel0 = dev.pos.clone(), dev.vel.clone()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(vel=dev.vel, dt=1.0, c1=1.0, c2=0.0, phase=3, n_sys=2):
        return lib.snet_mdb_step(P(dev.pos), P(vel), P(f), None, P(dev.mass), 69, P(dev.seg_ptr), P(dev.sys_id), n_sys, P(dev.kT),
                                 P(dev.step_index), P(dev.e_kin), dt, c1, c2, 0, phase, st)
    for kw in (dict(dt=0.0), dict(dt=-1.0), dict(c1=1.5), dict(c1=-0.1), dict(c2=-0.1), dict(c2=1.5), dict(phase=4), dict(phase=-1)):
        assert call(**kw) == 2 and b'out of range' in lib.snet_last_error(), kw
    assert call(vel=None) == 2 and b'null argument' in lib.snet_last_error()
    assert call(n_sys=0) == 2 and b'bad shape' in lib.snet_last_error()
    assert lib.snet_mdb_init_velocities(P(dev.vel), P(dev.mass), 69, P(dev.seg_ptr), P(dev.sys_id), 0, P(dev.kT), 0, 1, st) == 2
    assert lib.snet_mdb_init_velocities(P(dev.vel), None, 69, P(dev.seg_ptr), P(dev.sys_id), 2, P(dev.kT), 0, 1, st) == 2
    torch.cuda.synchronize()
    assert torch.equal(dev.pos, pos0) and torch.equal(dev.vel, vel0) and _h(dev.step_index).tolist() == [0, 0]
    with pytest.raises(ValueError, match='init_velocities'):   # the Python wrappers check dtypes and shapes before the call
        init_velocities(dev.vel, dev.mass.float(), dev.seg_ptr, dev.sys_id, dev.kT, 0)
    with pytest.raises(ValueError, match='md_step'):
        dev.step(np.zeros((68, 3)), 1.0, 1.0, 0.0, 0, 3)
    assert call() == 0


def test_a_systems_trajectory_does_not_depend_on_its_company():
    """systems [A, B, C] under ids [0, 1, 2] and C alone under id [2], five Langevin launches: C's pos / vel / e_kin bit for bit;
    under id [0] it sees other noise"""
    rng = np.random.default_rng(4)
    sizes = [64, 5, 300]
    masses = _masses(rng, sizes)
    kT = md_ref.KB * np.array([200.0, 300.0, 400.0])
    states = [md_ref.md_init(rng.normal(0, 0.5, (n, 3)), rng.normal(0, 0.01, (n, 3))) for n in sizes]
    c1, c2 = md_ref.langevin_coefficients(0.1, 0.5)

    def run(sel, ids):
        dev = _DeviceState([states[k] for k in sel], [masses[k] for k in sel], kT[sel], ids)
        for it in range(5):
            dev.step(_h((-2.0 * dev.pos).float()), 0.5, c1, c2, 9, 3 if it else 2)   # harmonic forces from the device state
        return dev
    full, alone, other = run([0, 1, 2], [0, 1, 2]), run([2], [2]), run([2], [0])
    lo = sizes[0] + sizes[1]
    assert torch.equal(full.pos[lo:], alone.pos) and torch.equal(full.vel[lo:], alone.vel) and torch.equal(full.e_kin[2:], alone.e_kin)
    assert not torch.equal(other.pos, alone.pos) and not torch.equal(other.vel, alone.vel)


def test_thermostat_reaches_its_temperature():
    """F = 0, v = 0, n = 3000, gamma dt = 0.1: after k O-steps every velocity component is N(0, kT ACC / m (1 - c1^2k)), so the
    temperature is T (1 - c1^2k) and its estimate from 3 n components scatters by sqrt(2 / (3 n)) relative: five of those"""
    n, T = 3000, 450.0
    rng = np.random.default_rng(8)
    masses = _masses(rng, [n])
    dev = _DeviceState([md_ref.md_init(np.zeros((n, 3)))], masses, [md_ref.KB * T])
    c1, c2 = md_ref.langevin_coefficients(0.1, 1.0)
    zero = np.zeros((n, 3))
    seen = {}
    for k in range(100):
        dev.step(zero, 1.0, c1, c2, 2024, md_ref.START)   # (e_kin of launch k: after k thermostat steps)
        if k in (1, 5, 20):
            seen[k] = float(dev.e_kin[0])
    dev.step(zero, 1.0, c1, c2, 2024, 0)
    seen[100] = float(dev.e_kin[0])
    assert _h(dev.step_index).tolist() == [100]
    for k, ek in seen.items():
        want, got = T * (1 - c1 ** (2 * k)), 2 * ek / (3 * n * md_ref.KB)
        print(f'after {k} steps: T {got:.2f} K, expected {want:.2f} K')
        assert abs(got - want) <= 5 * np.sqrt(2 / (3 * n)) * want, (k, got, want)


def test_init_velocities():
    from sevennet_amd.md import init_velocities
    rng = np.random.default_rng(6)
    masses = _masses(rng)
    kT = md_ref.KB * np.array([100.0, 300.0, 600.0, 1000.0])
    seg = _up(np.concatenate([[0], np.cumsum(SIZES)]), torch.int32)
    ids, seed = [4, 0, 9, 2], (5 << 32) | 6
    m_d, kT_d, id_d = _up(np.concatenate(masses), torch.float64), _up(kT, torch.float64), _up(ids, torch.int32)

    def draw(remove_com):
        vel = torch.full((sum(SIZES), 3), np.nan, dtype=torch.float64, device=DEV)
        init_velocities(vel, m_d, seg, id_d, kT_d, seed, remove_com)
        torch.cuda.synchronize()
        return vel
    a, b, raw = draw(True), draw(True), draw(False)
    assert torch.equal(a, b)
    sp = np.concatenate([[0], np.cumsum(SIZES)])
    for k, (n, m) in enumerate(zip(SIZES, masses)):
        v, r = _h(a)[sp[k]:sp[k + 1]], _h(raw)[sp[k]:sp[k + 1]]
        want_raw = md_ref.init_velocities(m, kT[k], seed, ids[k], remove_com=False)
        assert np.abs(r - want_raw).max() <= 1e-11 * np.abs(want_raw).max()
        if n == 1:
            assert not v.any() and r.any()
            continue
        want = md_ref.init_velocities(m, kT[k], seed, ids[k])
        assert np.abs(v - want).max() <= 1e-11 * np.abs(want).max(), k
        assert np.abs((m[:, None] * v).sum(0)).max() <= 1e-12 * (m[:, None] * np.abs(v)).sum(), k
        e_want = 0.5 * (3 * n - 3) * kT[k]
        assert abs(md_ref.kinetic_energy(m, v) - e_want) <= 1e-12 * e_want, k


# ------------------------------------------------------------------------------------------------ the driver on a model
@pytest.fixture(scope='module')
def model():
    from sevennet_amd.shapes import mini_sevennet_0_config
    calc, cfg, sd = _calc(mini_sevennet_0_config())
    return SimpleNamespace(calc=calc, cfg=cfg, sd=sd, orc=oracle_model(cfg, sd))


def _md_args(systems):
    z, pos, cells, pbcs = _args(systems)
    return z, pos, [MASS_OF[s[0]] for s in systems], cells, pbcs


def _start_velocities(systems, T=300.0):
    """Maxwell-Boltzmann at T from the restatement (centre of mass at rest); the isolated atom gets a velocity of its own"""
    return [md_ref.init_velocities(MASS_OF[s[0]], md_ref.KB * T, seed=100 + b, sys_id=b, remove_com=len(s[0]) > 1)
            for b, s in enumerate(systems)]


def _position_bound(t):
    """what a force error at the project's 1e-4 eV/A bar can displace in time t: (1/2) 1e-4 ACC / m_min t^2"""
    return 0.5 * 1e-4 * md_ref.ACC / MASS_OF.min() * t * t


def _oracle_runs(m, systems, vels, steps=STEPS):
    return [md_ref.md_run(pos, lambda p, s=(types, cell, pbc): _oracle(m, s[0], p, s[1], s[2]), MASS_OF[types], DT, steps, vel=v)
            for (types, pos, cell, pbc), v in zip(systems, vels)]


def test_first_steps_follow_the_fp64_oracle(model):
    systems = _all_systems()
    vels = _start_velocities(systems)
    res = model.calc.md_many(*_md_args(systems), DT, STEPS, velocities=vels, traj_every=1)
    ref = _oracle_runs(model, systems, vels)
    for b, (r, o) in enumerate(zip(res, ref)):
        assert r['trajectory'].shape == o['traj'].shape == (STEPS + 1,) + systems[b][1].shape
        for k in range(STEPS + 1):
            err = np.abs(r['trajectory'][k] - o['traj'][k]).max()
            assert err <= _position_bound(k * DT), (b, k, err)
        err = np.abs(r['positions'] - o['pos']).max()
        print(f'system {b}: max |dx| after {STEPS} steps {err:.3e} A (bound {_position_bound(STEPS * DT):.3e}), moved '
              f'{np.abs(o["pos"] - systems[b][1]).max():.3f} A; max |dv| {np.abs(r["velocities"] - o["vel"]).max():.3e} A/fs')
        assert np.array_equal(r['trajectory'][-1], r['positions'])
    atom, x0, v0 = res[-1], systems[-1][1], vels[-1]
    assert v0.any() and np.abs(atom['positions'] - (x0 + STEPS * DT * v0)).max() <= 1e-12 * np.abs(x0 + STEPS * DT * v0).max()   # free flight


def test_energy_is_conserved_as_well_as_the_integrator_allows(model):
    """NVE on MD-scaled weights: rescale_atomic_energy.scale chosen so that the first cell's largest force component is
    1.0 eV/A (tools/md_loop.md_scale_state), T = 300 K, dt = 1 fs, 12 steps, the three cells and the molecule.  Per system the
    largest excursion of e_pot + e_kin must stay within X_ref + 2e-5 max|e_pot|: X_ref is that of the restatement driven by the
    fp64 oracle (the integrator's own error), 1e-5 the project's energy-parity bar, applied to two samples.  Precondition: e_pot
    changes by more than 10 x the bound over the run, so a dropped half-kick or a sign error cannot pass.  With the oracle on the
    CPU: X_ref 1.06e-4 / 3.8e-5 / 1.16e-3 / 5.6e-5 eV, bounds 1.21e-3 / 7.8e-4 / 3.17e-3 / 5.7e-4 eV, |e_pot(end) - e_pot(0)|
    0.153 / 0.0243 / 0.625 / 0.0130 eV (126 / 31 / 197 / 23 x the bound).  The engine's runs on an MI355X, excursions:
    1.09e-4 / 3.83e-5 / 1.157e-3 / 5.68e-5 eV."""
    from md_loop import md_scale_state
    from sevennet_amd.calculator import SevenNetCalculator
    from sevennet_amd.neighbor import neighbor_list
    systems = _all_systems()[:4]
    t0, p0, c0, pbc0 = systems[0]
    ei, ev, _ = neighbor_list(p0, c0, pbc0, model.calc.cutoff)
    sdk = md_scale_state(model.cfg, model.sd, t0, ei, ev, 1.0)
    scaled = SimpleNamespace(calc=SevenNetCalculator((model.cfg, sdk), file_type='model_instance', device=DEV), orc=oracle_model(model.cfg, sdk))
    vels = _start_velocities(systems)
    ref = _oracle_runs(scaled, systems, vels)
    res = scaled.calc.md_many(*_md_args(systems), DT, STEPS, velocities=vels)
    for b, (r, o) in enumerate(zip(res, ref)):
        e_ref, e = o['e_pot'] + o['e_kin'], r['e_pot'] + r['e_kin']
        x_ref, x = np.abs(e_ref - e_ref[0]).max(), np.abs(e - e[0]).max()
        bound = x_ref + 2e-5 * np.abs(o['e_pot']).max()
        change = abs(o['e_pot'][-1] - o['e_pot'][0])
        print(f'system {b}: excursion {x:.3e} eV (oracle-driven {x_ref:.3e}, bound {bound:.3e}), e_pot changes by {change:.3e} eV')
        assert change > 10 * bound, (b, change, bound)
        assert x <= bound, (b, x, bound)


def test_determinism_and_the_noise_seed(model):
    systems = _all_systems()
    kw = dict(temperature=[300.0, 250.0, 350.0, 300.0, 300.0], friction=0.01, traj_every=6)
    a = model.calc.md_many(*_md_args(systems), DT, STEPS, seed=3, **kw)
    b = model.calc.md_many(*_md_args(systems), DT, STEPS, seed=3, **kw)
    c = model.calc.md_many(*_md_args(systems), DT, STEPS, seed=4, **kw)
    for x, y, z in zip(a, b, c):
        for k in ('positions', 'velocities', 'e_pot', 'e_kin', 'temperature', 'trajectory', 'forces'):
            assert np.array_equal(x[k], y[k]), k
        assert x['energy'] == y['energy'] and not np.array_equal(x['positions'], z['positions'])
    assert all(r['velocities'].any() for r in a)   # drawn at the temperature; the atom's by the thermostat
    alone = model.calc.md_many(*_md_args(systems[2:3]), DT, STEPS, seed=3, temperature=350.0, friction=0.01, system_ids=[2])
    err = np.abs(alone[0]['positions'] - a[2]['positions']).max()
    print(f'system 2 alone under its id: max |dx| {err:.3e} A (bound {_position_bound(STEPS * DT):.3e})')
    assert err <= _position_bound(STEPS * DT)
    moved = model.calc.md_many(*_md_args(systems[2:3]), DT, STEPS, seed=3, temperature=350.0, friction=0.01)   # id 0: other noise
    assert np.abs(moved[0]['positions'] - a[2]['positions']).max() > 100 * _position_bound(STEPS * DT)


def test_bookkeeping(model):
    systems = _all_systems()
    B = len(systems)
    vels = _start_velocities(systems)
    args = _md_args(systems)
    keep = [[np.array(x, copy=True) for x in part] for part in (args[0], args[1], args[2], vels)]
    res = model.calc.md_many(*args, DT, STEPS, velocities=vels)
    assert model.calc.md_info == dict(n_force_calls=STEPS + 1, md_launches=STEPS + 1, system_steps_evaluated=B * (STEPS + 1))
    for part, now in zip(keep, (args[0], args[1], args[2], vels)):
        assert all(np.array_equal(x, y) for x, y in zip(part, now))
    at = model.calc.compute_many(args[0], [r['positions'] for r in res], args[3], args[4])
    for b, (r, one) in enumerate(zip(res, at)):
        assert set(r) == set(one) | {'positions', 'velocities', 'e_pot', 'e_kin', 'temperature'}
        assert r['e_pot'].shape == r['e_kin'].shape == r['temperature'].shape == (STEPS + 1,)
        assert r['positions'].dtype == r['velocities'].dtype == np.float64 and r['positions'].shape == systems[b][1].shape
        assert abs(r['energy'] - one['energy']) <= 1e-6 * abs(one['energy']) + 1e-6, (b, r['energy'], one['energy'])
        assert np.abs(r['forces'] - one['forces']).max() <= 2e-5 * max(1.0, np.abs(one['forces']).max()), b
        assert r['e_pot'][-1] == r['energy']   # the last sample is the last engine call
        assert np.array_equal(r['temperature'], 2 * r['e_kin'] / (3 * len(systems[b][0]) * md_ref.KB))
        assert abs(r['e_kin'][0] - md_ref.kinetic_energy(MASS_OF[systems[b][0]], vels[b])) <= 1e-12 * r['e_kin'][0]
        assert abs(r['e_kin'][-1] - md_ref.kinetic_energy(MASS_OF[systems[b][0]], r['velocities'])) <= 1e-12 * r['e_kin'][-1]
    none = model.calc.md_many(*args, DT, 0, velocities=vels, traj_every=3)
    assert model.calc.md_info == dict(n_force_calls=1, md_launches=1, system_steps_evaluated=B)
    for b, r in enumerate(none):
        assert np.array_equal(r['positions'], systems[b][1]) and np.array_equal(r['velocities'], vels[b])
        assert r['e_pot'].shape == r['e_kin'].shape == (1,) and r['trajectory'].shape == (1,) + systems[b][1].shape
        assert np.isfinite(r['energy']) and np.isfinite(r['forces']).all() and np.isfinite(r['e_pot']).all() and np.isfinite(r['e_kin']).all()
        assert r['e_pot'][0] == res[b]['e_pot'][0] and r['e_kin'][0] == res[b]['e_kin'][0]
    sparse = model.calc.md_many(*args, DT, 14, velocities=vels, log_every=5, traj_every=4)
    assert model.calc.md_info['md_launches'] == 15
    for b, r in enumerate(sparse):
        assert r['e_pot'].shape == r['e_kin'].shape == (3,) and r['trajectory'].shape == (4,) + systems[b][1].shape   # steps 0 5 10; 0 4 8 12
        assert np.array_equal(r['e_pot'][:3], res[b]['e_pot'][[0, 5, 10]]) and np.array_equal(r['e_kin'][:3], res[b]['e_kin'][[0, 5, 10]])
        assert np.array_equal(r['trajectory'][0], systems[b][1]) and np.array_equal(r['trajectory'][3], res[b]['positions'])
        assert not np.array_equal(r['positions'], res[b]['positions'])   # (two steps further on)


class _Atoms:
    """what md_many_atoms reads from and writes to an ASE Atoms"""

    def __init__(self, z, pos, cell, pbc, masses, vel=None):
        self.z, self.pos, self.cell, self.pbc, self.masses = z, np.array(pos, float), cell, pbc, np.array(masses, float)
        self.vel = None if vel is None else np.array(vel, float)

    def get_atomic_numbers(self):
        return np.asarray(self.z)

    def get_positions(self):
        return self.pos.copy()

    def get_masses(self):
        return self.masses.copy()

    def get_velocities(self):
        return None if self.vel is None else self.vel.copy()

    def get_cell(self):
        return np.asarray(self.cell, float)

    def get_pbc(self):
        return np.asarray(self.pbc, bool)

    def set_positions(self, pos):
        self.pos = np.array(pos, float)

    def set_velocities(self, vel):
        self.vel = np.array(vel, float)


def test_surfaces(model):
    from sevennet_amd.d3 import SevenNetD3Calculator
    systems = _all_systems()
    vels = _start_velocities(systems)
    mk = lambda with_v: [_Atoms(np.array(Z)[s[0]], s[1], s[2], s[3], MASS_OF[s[0]], v if with_v else None)   # noqa: E731
                         for s, v in zip(systems, vels)]
    atoms = mk(True)
    res = model.calc.md_many_atoms(atoms, DT, 5)
    ref = model.calc.md_many(*_md_args(systems), DT, 5, velocities=vels)
    for a, r, q, s in zip(atoms, res, ref, systems):
        assert np.array_equal(a.get_positions(), r['positions']) and np.array_equal(r['positions'], q['positions'])
        assert np.array_equal(a.get_velocities(), r['velocities']) and np.array_equal(r['velocities'], q['velocities'])
    assert not np.array_equal(atoms[0].get_positions(), systems[0][1])
    cold = mk(False)   # no velocities on the objects: drawn at the temperature, and written back
    model.calc.md_many_atoms(cold, DT, 2, temperature=300.0, seed=1)
    assert all(a.get_velocities() is not None for a in cold) and cold[0].get_velocities().any()
    with pytest.raises(ValueError, match='neither velocities nor temperature'):
        model.calc.md_many_atoms(mk(False), DT, 2)
    with pytest.raises(ValueError, match='Model do not know atomic number: 79'):
        model.calc.md_many([[79]], [np.zeros((1, 3))], [[196.97]], np.zeros((1, 3, 3)), [False] * 3, DT, 1, temperature=300.0)
    d3 = SevenNetD3Calculator((model.cfg, model.sd), file_type='model_instance', device=DEV, **D3_CUT)
    cells = _cells()
    z, pos, masses, cs, pbcs = _md_args(cells)
    res = d3.md_many(z, pos, masses, cs, pbcs, DT, 3, velocities=vels[:3])
    assert d3.md_info == dict(n_force_calls=4, md_launches=4, system_steps_evaluated=12)
    plain = model.calc.md_many(z, pos, masses, cs, pbcs, DT, 3, velocities=vels[:3])
    for b, r in enumerate(res):
        one = d3.compute(z[b], r['positions'], cs[b], pbcs[b])
        assert abs(r['e_pot'][-1] - one['energy']) <= 1e-6 * abs(one['energy']) + 1e-6, (b, r['e_pot'][-1], one['energy'])
        assert abs(r['energy'] - one['energy']) <= 1e-6 * abs(one['energy']) + 1e-6
        assert np.abs(r['forces'] - one['forces']).max() <= 2e-5 * max(1.0, np.abs(one['forces']).max())
        assert set(r) == set(one) | {'positions', 'velocities', 'e_pot', 'e_kin', 'temperature'}
        assert r['e_pot'][0] != plain[b]['e_pot'][0] and not np.array_equal(r['positions'], plain[b]['positions'])   # D3 is in
    atoms = [_Atoms(np.array(Z)[s[0]], s[1], s[2], s[3], MASS_OF[s[0]], v) for s, v in zip(cells[:2], vels)]
    res = d3.md_many_atoms(atoms, DT, 2)
    assert all(np.array_equal(a.get_positions(), r['positions']) and np.array_equal(a.get_velocities(), r['velocities'])
               for a, r in zip(atoms, res))
