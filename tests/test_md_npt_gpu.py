"""GPU: constant-pressure batched MD -- the step kernel snet_mdb_npt_step against its fp64 restatement (md_npt_ref) on synthetic
forces and virials (systems of 1, 5, 64 and 3000 atoms, as in test_md_batch_gpu), and the driver and the public surfaces on a
model: the three rattled two-species diamond cells of the relax tests."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import md_npt_ref as ref
import md_ref
from test_batch_gpu import _calc
from test_md_batch_gpu import MASS_OF, SIZES, _position_bound
from test_md_npt_cpu import (B_GAS, GAS, GAS_DISCARD, GAS_STEPS, N_GAS, assert_gas_statistics, gas_start, gas_statistics)
from test_relax_gpu import D3_CUT, DEV, _args, _cells

pytestmark = pytest.mark.gpu

CAP, MIN_H = 0.1, 0.05


def _up(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _h(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the kernel
class _DeviceState:
    """the arrays of snet_mdb_npt_step for a list of md_npt_ref states"""

    def __init__(self, states, masses, kT, p0, beta_over_tau, sys_id=None):
        n = [len(s['pos']) for s in states]
        B = len(n)
        self.seg_ptr = _up(np.concatenate([[0], np.cumsum(n)]), torch.int32)
        self.pos = _up(np.concatenate([s['pos'] for s in states]), torch.float64)
        self.vel = _up(np.concatenate([s['vel'] for s in states]), torch.float64)
        self.cell = _up(np.stack([s['cell'].reshape(9) for s in states]), torch.float64)
        self.mass = _up(np.concatenate(masses), torch.float64)
        self.kT, self.p0, self.bt = (_up(np.broadcast_to(x, (B,)).copy(), torch.float64) for x in (kT, p0, beta_over_tau))
        self.sys_id = _up(np.arange(B) if sys_id is None else sys_id, torch.int32)
        self.step_index = _up([s['step'] for s in states], torch.int32)
        self.active = _up([s['active'] for s in states], torch.int32)
        self.status = _up([s['status'] for s in states], torch.int32)
        self.e_kin, self.volume, self.pressure = (torch.full((B,), -1.0, dtype=torch.float64, device=DEV) for _ in range(3))

    def step(self, forces32, virial, dt, c1, c2, seed, phase, extra=None, virial_extra=None, cap=CAP, min_h=MIN_H):
        from sevennet_amd.md import md_npt_step
        f, w = _up(forces32, torch.float32), _up(virial, torch.float64)
        x = None if extra is None else _up(extra, torch.float64)
        wx = None if virial_extra is None else _up(virial_extra, torch.float64)
        md_npt_step(self.pos, self.vel, self.cell, f, w, self.mass, self.seg_ptr, self.sys_id, self.kT, self.p0, self.bt,
                    self.step_index, self.e_kin, self.volume, self.pressure, self.active, self.status, dt, c1, c2, seed, phase, cap,
                    min_h, x, wx)
        torch.cuda.synchronize()

    def state_bits(self):
        return [t.clone() for t in (self.pos, self.vel, self.cell, self.step_index)]


def _masses(rng, sizes=SIZES):
    return [rng.choice([1.008, 15.999, 28.0855], n) for n in sizes]


def _cells_for(rng, sizes=SIZES):
    return [np.diag([9.0, 10.0, 11.0]) + rng.normal(0, 0.5, (3, 3)) for _ in sizes]


def _eos_virial(cell, v0, b0=0.4):
    """a virial that depends on the cell: trace 3 V b0 (1 - V / v0), and off-diagonal entries the pressure must not read"""
    v = abs(np.linalg.det(cell))
    d = v * b0 * (1.0 - v / v0)
    return np.array([d, 1.1 * d, 0.9 * d, 0.3, -0.2, 0.1])


def _compare(dev, states, outs, where):
    """pos / vel / cell to 1e-11 of each array's largest |component|, e_kin / volume / pressure to 1e-11 relative, the integer
    state exactly"""
    assert _h(dev.step_index).tolist() == [s['step'] for s in states], where
    assert _h(dev.active).tolist() == [s['active'] for s in states] and _h(dev.status).tolist() == [s['status'] for s in states], where
    for name, got in (('pos', _h(dev.pos)), ('vel', _h(dev.vel)), ('cell', _h(dev.cell).reshape(-1, 3))):
        want = np.concatenate([s[name] for s in states])
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        assert err <= 1e-11 * scale, (where, name, err, scale)
    for k, got in enumerate((_h(dev.e_kin), _h(dev.volume), _h(dev.pressure))):
        want = np.array([o[k] for o in outs])
        assert (np.abs(got - want) <= 1e-11 * np.abs(want)).all(), (where, ('e_kin', 'volume', 'pressure')[k], got, want)


@pytest.mark.parametrize('variant', ['nve', 'langevin', 'langevin_extras'])
def test_kernel_follows_the_restatement_step_by_step(variant):
    """40 steps in 41 launches, phase 2, 3, ..., 3, 1, the device state rebuilt from the restatement's each time.  The bound is
    that of test_md_batch_gpu: one fp64 sum of at most 9 000 terms in another order, 9 000 x 1.1e-16 ~ 1e-12, times 10; the
    volume's determinant and the exponential are a few ulp each.  nve: kT = 0 and c2 = 0 (no random number on either side);
    langevin_extras carries a second, fp64 force array and a second virial."""
    rng = np.random.default_rng(11)
    stiffness, dt, seed = [40.0, 3.0, 0.6, 5.0], 0.5, 77
    masses = _masses(rng)
    langevin, extras = variant != 'nve', variant == 'langevin_extras'
    kT = md_ref.KB * np.array([100.0, 300.0, 600.0, 1000.0]) if langevin else np.zeros(4)
    c1, c2 = md_ref.langevin_coefficients(0.1 if langevin else 0.0, dt)
    p0, bt = np.array([0.05, -0.02, 0.0, 0.1]), np.array([0.02, 0.05, 0.01, 0.03])
    cells = _cells_for(rng)
    v0 = [2.0 * abs(np.linalg.det(c)) for c in cells]
    states = [ref.npt_init(rng.normal(0, 0.5, (n, 3)), c, rng.normal(0, 0.01, (n, 3))) for n, c in zip(SIZES, cells)]
    n_launch = 41
    for it in range(n_launch):
        phase = md_ref.START if it == 0 else (md_ref.FINISH if it == n_launch - 1 else md_ref.FINISH | md_ref.START)
        f32 = [(-k * s['pos']).astype(np.float32) for k, s in zip(stiffness, states)]   # fp32, the same bits to both sides
        f64 = [1e-3 * np.sin(3.0 * s['pos']) if extras else 0.0 for s in states]
        w = np.stack([_eos_virial(s['cell'], v) for s, v in zip(states, v0)])
        wx = np.stack([0.05 * np.cos(s['cell'][0, :1] + np.arange(6.0)) for s in states]) if extras else None
        dev = _DeviceState(states, masses, kT, p0, bt)
        dev.step(np.concatenate(f32), w, dt, c1, c2, seed, phase, np.concatenate(f64) if extras else None, wx)
        nxt = [ref.npt_step(s, a.astype(np.float64) + x, w[b] + (wx[b] if extras else 0.0), masses[b], kT[b], p0[b], bt[b], dt, c1, c2,
                            seed, b, phase, CAP, MIN_H) for b, (s, a, x) in enumerate(zip(states, f32, f64))]
        states = [x[0] for x in nxt]
        _compare(dev, states, [x[1:] for x in nxt], (variant, it))
    assert [s['step'] for s in states] == [n_launch - 1] * 4 and all(s['status'] == 0 for s in states)
    moved = [abs(np.log(abs(np.linalg.det(s['cell'])) / abs(np.linalg.det(c)))) for s, c in zip(states, cells)]
    assert min(moved) > 1e-3, moved   # (the barostat did act on every system)


def test_barostat_noise_is_the_stated_noise():
    """v = 0, F = 0 and tr W = 3 V P0: the drift vanishes (to an ulp of P0), and 3 ln(cell_new / cell_old) of every cell entry is
    sqrt(2 kT beta dt / (V tau_p)) times the first normal of (atom word 0, system id, step, tag 2).  1e-13 absolute: the noise
    is at most 0.03 here, a few ulp of exp and log of numbers near 1 are 1e-15."""
    seed, steps0, ids = (0x9abcdef0 << 32) | 0x12345678, [0, 3, 17, 1000], [4, 0, 9, 2]
    rng = np.random.default_rng(2)
    cells = [np.diag([7.0, 8.0, 9.0]) + rng.normal(0, 0.5, (3, 3)) for _ in SIZES]
    kT, p0, bt, dt = np.full(4, 0.05), np.array([0.03, 0.0, -0.01, 0.2]), np.array([0.1, 0.05, 0.2, 0.1]), 1.0
    states = [ref.npt_init(rng.normal(0, 2.0, (n, 3)), c, step=k) for n, c, k in zip(SIZES, cells, steps0)]
    vol = np.array([abs(np.linalg.det(c)) for c in cells])
    w = np.zeros((4, 6))
    w[:, :3] = (vol * p0)[:, None]
    dev = _DeviceState(states, [np.ones(n) for n in SIZES], kT, p0, bt, ids)
    dev.step(np.zeros((sum(SIZES), 3)), w, dt, 1.0, 0.0, seed, md_ref.START)
    got = 3.0 * np.log(_h(dev.cell).reshape(4, 3, 3) / np.stack(cells))
    for b in range(4):
        xi = md_ref.normals(seed, ids[b], 1, steps0[b], 2)[0, 0]
        want = np.sqrt(2.0 * kT[b] * bt[b] * dt / vol[b]) * xi
        err = np.abs(got[b] - want).max()
        print(f'system id {ids[b]}, step {steps0[b]}: xi {xi:+.4f}, de {want:+.3e}, max |3 ln(cell ratio) - de| {err:.2e}')
        assert err <= 1e-13 and abs(want) > 1e-4, (b, err, want)
    assert _h(dev.step_index).tolist() == [k + 1 for k in steps0] and _h(dev.status).tolist() == [0] * 4
    other = _DeviceState(states, [np.ones(n) for n in SIZES], kT, p0, bt, ids)
    other.step(np.zeros((sum(SIZES), 3)), w, dt, 1.0, 0.0, seed + 1, md_ref.START)
    assert not torch.equal(other.cell, dev.cell)


@pytest.mark.parametrize('gamma_dt', [0.0, 0.05], ids=['nve', 'langevin'])
def test_without_coupling_the_kernel_is_snet_mdb_step_bit_for_bit(gamma_dt):
    """beta_over_tau = 0: mu is exactly 1, and over launches of phases 2, 3, 3, 3, 1 pos, vel, e_kin and step_index are those of
    snet_mdb_step on the same inputs, bit for bit; the cell does not change"""
    from sevennet_amd.md import md_step
    rng = np.random.default_rng(4)
    masses = _masses(rng)
    kT = md_ref.KB * np.array([100.0, 300.0, 600.0, 1000.0])
    dt, seed = 0.5, 31
    c1, c2 = md_ref.langevin_coefficients(gamma_dt / dt, dt)
    cells = _cells_for(rng)
    states = [ref.npt_init(rng.normal(0, 0.5, (n, 3)), c, rng.normal(0, 0.01, (n, 3))) for n, c in zip(SIZES, cells)]
    a = _DeviceState(states, masses, kT, 0.05, 0.0)
    pos, vel, step_index, e_kin = a.pos.clone(), a.vel.clone(), a.step_index.clone(), torch.zeros_like(a.e_kin)
    cell0 = a.cell.clone()
    for phase in (2, 3, 3, 3, 1):
        f32 = (-2.0 * a.pos).float()
        fx = (1e-3 * torch.sin(3.0 * a.pos)).contiguous()
        w = rng.normal(0, 5.0, (4, 6))
        md_step(pos, vel, f32, a.mass, a.seg_ptr, a.sys_id, a.kT, step_index, e_kin, dt, c1, c2, seed, phase, fx)
        a.step(_h(f32), w, dt, c1, c2, seed, phase, _h(fx))
        assert torch.equal(a.pos, pos) and torch.equal(a.vel, vel) and torch.equal(a.e_kin, e_kin), phase
        assert torch.equal(a.step_index, step_index) and torch.equal(a.cell, cell0), phase
    assert _h(step_index).tolist() == [4] * 4 and not torch.equal(pos, _up(np.concatenate([s['pos'] for s in states]), torch.float64))
    assert _h(a.status).tolist() == [0] * 4 and _h(a.active).tolist() == [1] * 4


def test_guard_refuses_and_keeps_every_bit():
    """A NaN virial, a virial that drives |de| beyond the cap and a cell one step from min_height are refused: status 2, active 0,
    pos / vel / cell / step_index keep their bits (the finishing kick is not stored either), in that launch and in the next;
    the fourth system of the batch moves as the restatement says.  A system that enters with active = 0 keeps every bit too."""
    rng = np.random.default_rng(9)
    sizes = [5, 300, 64, 40]
    masses = _masses(rng, sizes)
    dt, seed, min_h = 0.5, 3, 2.0
    c1, c2 = md_ref.langevin_coefficients(0.1, dt)
    kT, p0, bt = np.full(4, md_ref.KB * 300.0), np.full(4, 0.01), np.full(4, 0.02)
    cells = [np.diag([9.0, 10.0, 11.0]), np.diag([9.0, 10.0, 11.0]), np.diag([9.0, 10.0, 2.001]), np.diag([9.0, 10.0, 11.0])]
    states = [ref.npt_init(rng.normal(0, 0.5, (n, 3)), c, rng.normal(0, 0.01, (n, 3)), step=7) for n, c in zip(sizes, cells)]
    w = np.zeros((4, 6))
    w[0, 1] = np.nan
    w[1, :3] = 1e5          # P ~ 100 eV/A^3: de = 0.02 x 100 x 0.5 = 1 > 0.1
    w[2, :3] = -60.0        # P ~ -0.33: de ~ -3e-3, the 2.001 A height falls below 2.0 (the noise is 3e-4 at most)
    w[3, :3] = 20.0
    f32 = rng.normal(0, 1.0, (sum(sizes), 3)).astype(np.float32)
    sp = np.concatenate([[0], np.cumsum(sizes)])
    dev = _DeviceState(states, masses, kT, p0, bt)
    before = dev.state_bits()
    dev.step(f32, w, dt, c1, c2, seed, 3, min_h=min_h)
    nxt = [ref.npt_step(s, f32[sp[b]:sp[b + 1]], w[b], masses[b], kT[b], p0[b], bt[b], dt, c1, c2, seed, b, 3, CAP, min_h)
           for b, s in enumerate(states)]
    assert [x[0]['status'] for x in nxt] == [2, 2, 2, 0]
    assert _h(dev.status).tolist() == [2, 2, 2, 0] and _h(dev.active).tolist() == [0, 0, 0, 1]
    lo = sp[3]

    def kept(now):
        return (torch.equal(now[0][:lo], before[0][:lo]) and torch.equal(now[1][:lo], before[1][:lo])
                and torch.equal(now[2][:3], before[2][:3]) and torch.equal(now[3][:3], before[3][:3]))
    assert kept(dev.state_bits())
    healthy = nxt[3][0]
    for name, got in (('pos', _h(dev.pos)[lo:]), ('vel', _h(dev.vel)[lo:]), ('cell', _h(dev.cell)[3].reshape(3, 3))):
        assert np.abs(got - healthy[name]).max() <= 1e-11 * np.abs(healthy[name]).max(), name
    assert int(dev.step_index[3]) == 8 == healthy['step'] and not np.array_equal(healthy['cell'], cells[3])
    ek = np.array([x[1] for x in nxt])
    assert (np.abs(_h(dev.e_kin) - ek) <= 1e-11 * ek).all()   # (of the refused: the kinetic energy the refusal was decided on)
    assert np.isnan(float(dev.pressure[0])) and abs(float(dev.pressure[3]) - nxt[3][3]) <= 1e-11 * abs(nxt[3][3])
    # a further launch on a harmless virial: the refused stay as they are, and are still measured
    w2 = np.zeros((4, 6))
    w2[:, :3] = 20.0
    dev.step(f32, w2, dt, c1, c2, seed, 3, min_h=min_h)
    assert kept(dev.state_bits()) and _h(dev.status).tolist() == [2, 2, 2, 0] and _h(dev.active).tolist() == [0, 0, 0, 1]
    assert int(dev.step_index[3]) == 9
    ek = np.array([md_ref.kinetic_energy(m, s['vel']) for m, s in zip(masses[:3], states[:3])])
    assert (np.abs(_h(dev.e_kin)[:3] - ek) <= 1e-11 * ek).all() and np.isfinite(_h(dev.pressure)).all()
    # active = 0 at entry, whatever the status word says
    idle = _DeviceState([dict(s, active=0) for s in states], masses, kT, p0, bt)
    before = idle.state_bits()
    idle.step(f32, w2, dt, c1, c2, seed, 3, min_h=min_h)
    assert all(torch.equal(x, y) for x, y in zip(idle.state_bits(), before))
    assert _h(idle.status).tolist() == [0] * 4 and _h(idle.active).tolist() == [0] * 4 and (_h(idle.volume) > 0).all()


def test_entry_point_checks_its_ranges():
    import ctypes as C
    from sevennet_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(2)
    states = [ref.npt_init(rng.normal(0, 0.5, (n, 3)), np.eye(3) * 9.0, rng.normal(0, 0.01, (n, 3))) for n in (5, 64)]
    dev = _DeviceState(states, _masses(rng, (5, 64)), 0.02, 0.01, 0.02)
    f, w = _up(np.zeros((69, 3)), torch.float32), _up(np.zeros((2, 6)), torch.float64)
    before = dev.state_bits()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(cell=dev.cell, dt=1.0, c1=1.0, c2=0.0, phase=3, n_sys=2, cap=0.1, min_h=0.1):
        return lib.snet_mdb_npt_step(P(dev.pos), P(dev.vel), P(cell), P(f), None, P(w), None, P(dev.mass), 69, P(dev.seg_ptr),
                                     P(dev.sys_id), n_sys, P(dev.kT), P(dev.p0), P(dev.bt), P(dev.step_index), P(dev.e_kin),
                                     P(dev.volume), P(dev.pressure), P(dev.active), P(dev.status), dt, c1, c2, 0, phase, cap, min_h, st)
    for kw in (dict(dt=0.0), dict(c1=1.5), dict(c2=-0.1), dict(phase=4), dict(phase=-1), dict(cap=0.0), dict(cap=float('nan')),
               dict(min_h=-1.0)):
        assert call(**kw) == 2 and b'out of range' in lib.snet_last_error(), kw
    assert call(cell=None) == 2 and b'null argument' in lib.snet_last_error()
    assert call(n_sys=0) == 2 and b'bad shape' in lib.snet_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(dev.state_bits(), before))
    with pytest.raises(ValueError, match='md_npt_step'):
        dev.step(np.zeros((69, 3)), np.zeros((2, 5)), 1.0, 1.0, 0.0, 0, 3)
    assert call() == 0
    torch.cuda.synchronize()


def test_ideal_gas_on_the_device():
    """test_md_npt_cpu's ideal gas through the kernel: 3001 launches on zero forces and virials, no model, the volumes logged on
    the device.  The same assertions (mean within 4 standard errors, variance within 10 %), and the device's mean within one
    standard error of the restatement's at the same seed -- the two runs see the same noise, and differ by rounding that the
    thermostat's contraction forgets.  On an MI355X: mean / exact 1.00885 on both sides at a standard error of 0.00779, variance /
    exact 1.0181, smallest volume 54.4 A^3; the first 20 steps agree to 3e-15 relative."""
    from sevennet_amd.md import md_npt_step
    c1, c2 = md_ref.langevin_coefficients(0.05, GAS['dt'])
    pos, vel, cells = gas_start()
    states = [ref.npt_init(p, c, v) for p, v, c in zip(pos, vel, cells)]
    dev = _DeviceState(states, [GAS['mass']] * B_GAS, GAS['kT'], GAS['p0'], GAS['beta_over_tau'])
    f = torch.zeros(B_GAS * N_GAS, 3, dtype=torch.float32, device=DEV)
    w = torch.zeros(B_GAS, 6, dtype=torch.float64, device=DEV)
    log = torch.zeros(GAS_STEPS + 1, B_GAS, dtype=torch.float64, device=DEV)
    for k in range(GAS_STEPS + 1):
        md_npt_step(dev.pos, dev.vel, dev.cell, f, w, dev.mass, dev.seg_ptr, dev.sys_id, dev.kT, dev.p0, dev.bt, dev.step_index,
                    dev.e_kin, dev.volume, dev.pressure, dev.active, dev.status, GAS['dt'], c1, c2, GAS['seed'],
                    (1 if k else 0) | (2 if k < GAS_STEPS else 0), GAS['max_log_volume_step'], GAS['min_height_bound'])
        log[k].copy_(dev.volume)
    vol = _h(log)
    assert _h(dev.status).tolist() == [0] * B_GAS and _h(dev.step_index).tolist() == [GAS_STEPS] * B_GAS
    mean, se = assert_gas_statistics(vol[GAS_DISCARD:], 'device')
    want = ref.free_gas_run(pos, vel, cells, c1=c1, c2=c2, sys_ids=np.arange(B_GAS), steps=GAS_STEPS, **GAS)[3]
    mean_ref = gas_statistics(want[GAS_DISCARD:])[0]
    print(f'device mean / exact {mean:.5f}, restatement {mean_ref:.5f}, standard error {se:.5f}; first 20 steps agree to '
          f'{np.abs(vol[:21] / want[:21] - 1).max():.1e}')
    assert abs(mean - mean_ref) <= se
    assert np.abs(vol[:21] / want[:21] - 1).max() <= 1e-11


# ------------------------------------------------------------------------------------------------ the driver on a model
@pytest.fixture(scope='module')
def model():
    from sevennet_amd.shapes import mini_sevennet_0_config
    calc, cfg, sd = _calc(mini_sevennet_0_config())
    return SimpleNamespace(calc=calc, cfg=cfg, sd=sd)


DT, STEPS = 1.0, 12
NPT = dict(pressure=0.01, compressibility=50.0, barostat_time=100.0)


def _md_args(systems):
    z, pos, cells, pbcs = _args(systems)
    return z, pos, [MASS_OF[s[0]] for s in systems], cells, pbcs


def _start_velocities(systems, T=300.0):
    return [md_ref.init_velocities(MASS_OF[s[0]], md_ref.KB * T, seed=100 + b, sys_id=b) for b, s in enumerate(systems)]


def _virial(res, cell):
    """the engine's virial (xx,yy,zz,xy,yz,zx) back from a results dict's stress"""
    return -res['stress'][[0, 1, 2, 5, 3, 4]] * abs(np.linalg.det(cell))


# |fp64 oracle - fp32 oracle| of the restatement's cell entries (A) after STEPS steps, per cell
ORACLE_CELL_SPREAD = [5.88e-9, 4.30e-9, 8.43e-9]


def test_first_steps_follow_the_restatement_on_the_model(model):
    """12 steps on the device (300 K, start velocities from md_ref.init_velocities, friction 0.01 / fs, P0 = 0.01 eV/A^3, beta =
    50 A^3/eV, tau_p = 100 fs) against the restatement driven by calc.compute_many at the restatement's own state: all three
    cells in one call per step, as in the loop.  Positions within the bound of test_md_batch_gpu (a force error at the 1e-4 eV/A
    bar over the time run).  The cell bound is measured, not assumed: the restatement was run on the CPU with the fp64 oracle and
    with the fp32 oracle from the same start; after 12 steps the two differ by 5.88e-9 / 4.30e-9 / 8.43e-9 A in the cell entries
    (ORACLE_CELL_SPREAD) and by 4.53e-9 / 3.46e-9 / 7.37e-9 A in the positions, while the cell entries moved 0.048 / 0.094 /
    0.170 A (volumes 160.19 -> 155.98, 160.19 -> 152.01, 320.38 -> 305.56 A^3; the largest |de| of a step 0.020).  That is what
    single precision in the force call is worth over these steps; 1.5 times it is allowed.  Precondition: the cell entries and the
    volume change by more than 10 times that bound, so a dropped barostat term cannot pass."""
    systems = _cells()
    z, pos, masses, cells, pbcs = _md_args(systems)
    vels = _start_velocities(systems)
    kw = dict(velocities=vels, temperature=300.0, friction=0.01, seed=5, **NPT)
    res = model.calc.md_many(z, pos, masses, cells, pbcs, DT, STEPS, traj_every=1, **kw)
    c1, c2 = md_ref.langevin_coefficients(0.01, DT)
    kT, bt = md_ref.KB * 300.0, NPT['compressibility'] / NPT['barostat_time']
    states = [ref.npt_init(p, c, v) for p, c, v in zip(pos, cells, vels)]
    for k in range(STEPS + 1):
        for b, (r, s) in enumerate(zip(res, states)):
            err = np.abs(r['trajectory'][k] - s['pos']).max()
            assert err <= _position_bound(k * DT), (b, k, err)
        out = model.calc.compute_many(z, [s['pos'] for s in states], np.stack([s['cell'] for s in states]), pbcs)
        phase = (md_ref.FINISH if k > 0 else 0) | (md_ref.START if k < STEPS else 0)
        states = [ref.npt_step(s, o['forces'], _virial(o, s['cell']), masses[b], kT, NPT['pressure'], bt, DT, c1, c2, 5, b, phase, 0.1,
                               model.calc.cutoff / 64)[0] for b, (s, o) in enumerate(zip(states, out))]
    for b, (r, s) in enumerate(zip(res, states)):
        tol = 1.5 * ORACLE_CELL_SPREAD[b]
        e_pos, e_cell, moved = np.abs(r['positions'] - s['pos']).max(), np.abs(r['cell'] - s['cell']).max(), np.abs(r['cell'] - cells[b]).max()
        dv = abs(r['volume'][-1] - r['volume'][0])
        print(f'cell {b}: max |dx| {e_pos:.3e} A (bound {_position_bound(STEPS * DT):.3e}), max |dC| {e_cell:.3e} A (bound {tol:.2e}), '
              f'cell moved {moved:.3e} A, volume {r["volume"][0]:.3f} -> {r["volume"][-1]:.3f} A^3')
        assert r['status'] == 'ok' and s['status'] == 0 and s['step'] == STEPS
        assert moved > 10 * tol and dv > 10 * tol, (b, moved, dv, tol)   # a dropped barostat term cannot pass
        assert e_pos <= _position_bound(STEPS * DT), (b, e_pos)
        assert e_cell <= tol, (b, e_cell, tol)


def test_sign_of_the_coupling(model):
    """kT = 0, atoms at rest at the start, friction 0.05 / fs, 30 steps: under +0.05 eV/A^3 every logged volume is below the one
    before, under -0.05 above; and at P0 = the pressure of the first sample the first de is zero"""
    systems = _cells()
    z, pos, masses, cells, pbcs = _md_args(systems)
    kw = dict(velocities=[np.zeros_like(p) for p in pos], temperature=0.0, friction=0.05, compressibility=50.0, barostat_time=500.0)
    down = model.calc.md_many(z, pos, masses, cells, pbcs, DT, 30, pressure=0.05, **kw)
    up = model.calc.md_many(z, pos, masses, cells, pbcs, DT, 30, pressure=-0.05, **kw)
    for b, (d, u) in enumerate(zip(down, up)):
        print(f'cell {b}: P(0) {d["pressure"][0]:+.4f} eV/A^3, volume {d["volume"][0]:.2f} -> {d["volume"][-1]:.2f} under +0.05, '
              f'-> {u["volume"][-1]:.2f} under -0.05')
        assert d['status'] == u['status'] == 'ok' and d['volume'].shape == (31,)
        assert d['volume'][0] == u['volume'][0] and d['pressure'][0] == u['pressure'][0]
        assert abs(d['volume'][0] - abs(np.linalg.det(cells[b]))) <= 1e-14 * d['volume'][0]
        assert (np.diff(d['volume']) < 0).all(), (b, d['volume'])
        assert (np.diff(u['volume']) > 0).all(), (b, u['volume'])
    still = model.calc.md_many(z, pos, masses, cells, pbcs, DT, 1, pressure=[d['pressure'][0] for d in down], **kw)
    for b, r in enumerate(still):
        de = np.log(r['volume'][1] / r['volume'][0])
        assert abs(de) <= 1e-12, (b, de)


def test_results_belong_to_the_returned_state(model):
    systems = _cells()
    z, pos, masses, cells, pbcs = _md_args(systems)
    keep = [np.array(c, copy=True) for c in cells]
    res = model.calc.md_many(z, pos, masses, cells, pbcs, DT, STEPS, temperature=300.0, friction=0.01, seed=5, log_every=4, **NPT)
    assert model.calc.md_info == dict(n_force_calls=STEPS + 1, md_launches=STEPS + 1, system_steps_evaluated=3 * (STEPS + 1))
    assert all(np.array_equal(a, b) for a, b in zip(keep, cells))
    at = model.calc.compute_many(z, [r['positions'] for r in res], np.stack([r['cell'] for r in res]), pbcs)
    for b, (r, one) in enumerate(zip(res, at)):
        assert set(r) == set(one) | {'positions', 'velocities', 'e_pot', 'e_kin', 'temperature', 'cell', 'volume', 'pressure', 'status'}
        assert r['volume'].shape == r['pressure'].shape == r['e_kin'].shape == (STEPS // 4 + 1,) and r['cell'].shape == (3, 3)
        assert r['cell'].dtype == r['volume'].dtype == r['pressure'].dtype == np.float64 and r['status'] == 'ok'
        assert not np.array_equal(r['cell'], cells[b])
        assert r['energy'] == one['energy'] and np.array_equal(r['forces'], one['forces']) and np.array_equal(r['stress'], one['stress'])
        vol = abs(np.linalg.det(r['cell']))
        p_want = 2.0 * r['e_kin'][-1] / (3.0 * vol) - r['stress'][:3].sum() / 3.0
        assert abs(r['volume'][-1] - vol) <= 1e-10 * vol
        assert abs(r['pressure'][-1] - p_want) <= 1e-10 * abs(p_want), (b, r['pressure'][-1], p_want)
        assert abs(r['e_kin'][-1] - md_ref.kinetic_energy(masses[b], r['velocities'])) <= 1e-12 * r['e_kin'][-1]
        assert r['e_pot'][-1] == r['energy']


def test_alone_equals_in_the_batch_and_twice_equals_once(model):
    systems = _cells()
    z, pos, masses, cells, pbcs = _md_args(systems)
    kw = dict(temperature=[300.0, 250.0, 350.0], friction=0.01, **NPT)
    a = model.calc.md_many(z, pos, masses, cells, pbcs, DT, STEPS, seed=3, **kw)
    b = model.calc.md_many(z, pos, masses, cells, pbcs, DT, STEPS, seed=3, **kw)
    c = model.calc.md_many(z, pos, masses, cells, pbcs, DT, STEPS, seed=4, **kw)
    keys = ('positions', 'velocities', 'cell', 'volume', 'pressure', 'e_pot', 'e_kin', 'forces', 'stress')
    for x, y, other in zip(a, b, c):
        for k in keys:
            assert np.array_equal(x[k], y[k]), k
        assert not np.array_equal(x['cell'], other['cell'])
    alone = model.calc.md_many(z[2:3], pos[2:3], masses[2:3], cells[2:3], pbcs[2:3], DT, STEPS, seed=3, system_ids=[2],
                               **dict(kw, temperature=350.0))[0]
    for k in keys:
        print(f'system 2 alone under its id, {k}: max |difference| {np.abs(alone[k] - a[2][k]).max():.3e}')
    for k in keys:
        assert np.array_equal(alone[k], a[2][k]), k
    moved = model.calc.md_many(z[2:3], pos[2:3], masses[2:3], cells[2:3], pbcs[2:3], DT, STEPS, seed=3,
                               **dict(kw, temperature=350.0))[0]   # id 0: other noise
    assert not np.array_equal(moved['cell'], a[2]['cell'])


def test_d3_device_term_under_pressure(model):
    from sevennet_amd.d3 import SevenNetD3Calculator
    d3 = SevenNetD3Calculator((model.cfg, model.sd), file_type='model_instance', device=DEV, **D3_CUT)
    systems = _cells()
    z, pos, masses, cells, pbcs = _md_args(systems)
    vels = _start_velocities(systems)
    kw = dict(velocities=vels, temperature=300.0, friction=0.01, seed=5, **NPT)
    with pytest.raises(ValueError, match='no virial'):
        d3.md_many(z, pos, masses, cells, pbcs, DT, 6, d3_term='host', **kw)
    res = d3.md_many(z, pos, masses, cells, pbcs, DT, 6, d3_term='device', **kw)
    assert d3.md_info == dict(n_force_calls=7, md_launches=7, system_steps_evaluated=21)
    plain = model.calc.md_many(z, pos, masses, cells, pbcs, DT, 6, **kw)
    start = d3.compute_many(z, pos, cells, pbcs)
    c1, c2 = md_ref.langevin_coefficients(0.01, DT)
    at_cells = d3.compute_many(z, [r['positions'] for r in res], np.stack([r['cell'] for r in res]), pbcs)
    at_old = d3.compute_many(z, [r['positions'] for r in res], cells, pbcs)
    for b, r in enumerate(res):
        s = ref.npt_init(pos[b], cells[b], vels[b])
        nxt, _, vol, pr = ref.npt_step(s, start[b]['forces'], _virial(start[b], cells[b]), masses[b], md_ref.KB * 300.0, NPT['pressure'],
                                       0.5, DT, c1, c2, 5, b, md_ref.START, 0.1, model.calc.cutoff / 64)
        de_ref = np.log(abs(np.linalg.det(nxt['cell'])) / vol)
        de = np.log(r['volume'][1] / r['volume'][0])
        print(f'cell {b}: first de {de:+.6e} (restatement {de_ref:+.6e}, model alone {np.log(plain[b]["volume"][1] / plain[b]["volume"][0]):+.6e}), '
              f'P(0) {r["pressure"][0]:+.5f} against {pr:+.5f}')
        assert r['status'] == 'ok' and abs(de - de_ref) <= 1e-9 * abs(de_ref), (b, de, de_ref)
        assert r['pressure'][0] != plain[b]['pressure'][0]   # the D3 virial is in
        one, old = at_cells[b], at_old[b]
        assert abs(r['energy'] - one['energy']) <= 1e-6 * abs(one['energy']) + 1e-6, (b, r['energy'], one['energy'])
        assert np.abs(r['stress'] - one['stress']).max() <= 1e-5 * max(1e-3, np.abs(one['stress']).max()), b
        assert np.abs(r['stress'] - old['stress']).max() > 1e-5 * max(1e-3, np.abs(one['stress']).max()), b   # (not at the caller's cell)


def test_without_a_pressure_the_run_is_the_fixed_cell_path(model, monkeypatch):
    from sevennet_amd import _lib
    real = _lib.load()
    calls = dict(snet_mdb_step=0, snet_mdb_npt_step=0)

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in calls:
                return fn

            def counted(*a):
                calls[name] += 1
                return fn(*a)
            return counted
    monkeypatch.setattr(_lib, 'load', lambda: Counting())
    systems = _cells()
    z, pos, masses, cells, pbcs = _md_args(systems)
    vels = _start_velocities(systems)
    res = model.calc.md_many(z, pos, masses, cells, pbcs, DT, 5, velocities=vels)
    assert calls == dict(snet_mdb_step=6, snet_mdb_npt_step=0)
    assert all(not {'cell', 'status', 'volume', 'pressure'} & set(r) for r in res)
    model.calc.md_many(z, pos, masses, cells, pbcs, DT, 5, velocities=vels, temperature=300.0, **NPT)
    assert calls == dict(snet_mdb_step=6, snet_mdb_npt_step=6)
