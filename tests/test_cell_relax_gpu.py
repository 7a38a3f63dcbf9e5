"""GPU: variable-cell FIRE relaxation -- the step kernel against its fp64 restatement (cellrelax_ref) step by step, its guard, the
driver on an analytic energy with a known minimum (cellrelax_ref.harmonic_crystal) and on a model: the three rattled two-species
diamond cells of test_relax_gpu, strained by the symmetric EPS (up to 3 %).

Random weights have no repulsion, so convergence on the model was searched on the CPU first (the fp64 oracle driving the
restatement, 200 evaluations at most, guard at cutoff / 64, strains EPS and EPS / 2, pressures 0 / 0.02 / 0.05 eV/A^3, fmax 0.05
and 0.02 eV/A): see test_model_convergence for what was found."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cellrelax_ref as ref
from test_batch_gpu import Z, _calc
from test_relax_gpu import _args, _cells

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FMAX = 0.02
C0 = np.array([[4.1, 0.0, 0.0], [0.7, 3.8, 0.0], [-0.5, 0.9, 4.3]])                       # triclinic
F_INIT = np.array([[1.04, 0.03, -0.02], [0.01, 0.97, 0.05], [0.02, -0.04, 1.06]])        # condition number 1.13
EPS = np.array([[0.03, 0.01, 0.0], [0.01, -0.02, 0.015], [0.0, 0.015, 0.025]])
SIZES, K_ATOM, K_CELL = [1, 5, 64, 300], [40.0, 3.0, 0.6, 5.0], [30.0, 8.0, 1.5, 4.0]
VARIANTS = {'plain': {}, 'pressure_mask': dict(scalar_pressure=0.02, cell_mask=[1, 1, 0, 1, 0, 1]), 'extras': {}}


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


# ------------------------------------------------------------------------------------------------ the kernel
def _initial_states(seed=11):
    rng = np.random.default_rng(seed)
    return [ref.cell_fire_init(rng.normal(0, 0.5, (n, 3)), C0 @ F_INIT.T, cell0=C0) for n in SIZES]


def _synthetic(states, variant):
    """forces pulling the atoms to the origin and a symmetric virial pulling F to I -> per system (forces fp32, virial fp64[6],
    forces_extra, virial_extra); fp32 forces and fp64 virials go to both sides with the same bits"""
    out = []
    for s, ka, kc in zip(states, K_ATOM, K_CELL):
        n = len(s['pos'])
        E = ref.deformation(s['cell'], s['cell0']) - np.eye(3)
        w = np.array(ref.virial6(-kc * n * 0.5 * (E + E.T)))
        fx = wx = None
        if variant == 'extras':
            fx = 1e-3 * np.sin(3.0 * s['pos'])
            wx = np.array(ref.virial6(0.02 * n * np.cos(s['cell'] + s['cell'].T)))
        out.append(((-ka * s['pos']).astype(np.float32), w, fx, wx))
    return out


class _DeviceState:
    """the per-system arrays of snet_fire_cell_step for a list of cellrelax_ref states"""

    def __init__(self, states):
        n = [len(s['pos']) for s in states]
        f64, i32 = torch.float64, torch.int32
        self.seg_ptr = _t(np.concatenate([[0], np.cumsum(n)]), i32)
        self.pos = _t(np.concatenate([s['pos'] for s in states]), f64)
        self.vel = _t(np.concatenate([s['vel'] for s in states]), f64)
        self.cell = _t(np.stack([s['cell'].reshape(9) for s in states]), f64)
        self.cell0 = _t(np.stack([s['cell0'].reshape(9) for s in states]), f64)
        self.vel_cell = _t(np.stack([s['vel_cell'].reshape(9) for s in states]), f64)
        self.dt = _t([s['dt'] for s in states], f64)
        self.alpha = _t([s['alpha'] for s in states], f64)
        self.n_pos = _t([s['n_pos'] for s in states], i32)
        self.active = _t([s['active'] for s in states], i32)
        self.n_steps = _t([s['n_steps'] for s in states], i32)
        self.status = _t([s['status'] for s in states], i32)
        self.fmax_sys = torch.full((len(n),), -1.0, dtype=f64, device=DEV)
        self.n_active = torch.full((1,), -1, dtype=i32, device=DEV)

    def step(self, forces32, virial, fmax, min_h=0.0, extra=None, virial_extra=None, opts=None, **fire):
        from sevennet_amd.relax import check_cell_params, check_fire_params, fire_cell_step
        x = None if extra is None else _t(extra, torch.float64)
        wx = None if virial_extra is None else _t(virial_extra, torch.float64)
        fire_cell_step(self.pos, self.vel, self.cell, self.vel_cell, self.cell0, _t(forces32, torch.float32), _t(virial, torch.float64),
                       self.seg_ptr, self.dt, self.alpha, self.n_pos, self.active, self.n_steps, self.status, self.fmax_sys,
                       self.n_active, fmax, check_fire_params(fmax, 1, 0.5, fire),
                       check_cell_params(**dict(ref.CELL, **(opts or {}))), min_h, x, wx)
        torch.cuda.synchronize()


def _compare(dev, states, what):
    """device state after one step against the restatement's next states: integers, dt and alpha exactly; pos, vel, cell and
    vel_cell to 1e-11 of the array's largest |component|.  Derivation, as test_relax_gpu._compare: the four fp64 sums over the
    rows, here of at most 303 x 3 terms in another order, are off by at most 909 x 1.1e-16 = 1e-13 relative; on top come 3 x 3
    products (three terms each: 3 x 1.1e-16 per product, a chain of at most five of them from C to the new positions) and two
    inverses by cofactors against LAPACK's (C0 and F with condition numbers 1.4 and under 2: 2 x 10 x 1.1e-16 each), together
    under 1e-14.  The sum is 1.1e-13, times the same factor 10 of safety 1.1e-12: the existing 1e-11 holds and is kept."""
    h = lambda t: t.cpu().numpy()   # noqa: E731
    for name in ('n_pos', 'active', 'n_steps', 'status', 'dt', 'alpha'):
        assert h(getattr(dev, name)).tolist() == [s[name] for s in states], name
    assert int(dev.n_active.item()) == sum(s['active'] for s in states)
    for name, got in (('pos', h(dev.pos)), ('vel', h(dev.vel)), ('cell', h(dev.cell)), ('vel_cell', h(dev.vel_cell))):
        want = np.concatenate([s[name].reshape(-1, 3) for s in states])
        err, scale = np.abs(got.reshape(-1, 3) - want).max(), np.abs(want).max()
        assert err <= 1e-11 * scale, (name, err, scale)
    fm = h(dev.fmax_sys)
    for k, w in enumerate(what):
        if w['fm'] is not None:   # the system was active going in
            assert abs(fm[k] - w['fm']) <= 1e-13 * max(w['fm'], 1e-300), (k, fm[k], w['fm'])


def _kernel_sequence(variant, check=True, steps=60):
    """`steps` steps of the four systems, the restatement next to the kernel -> what was seen"""
    states = _initial_states()
    opts = VARIANTS[variant]
    seen = {'uphill': 0, 'downhill': 0, 'clipped': 0, 'frozen': 0, 'guard': 0}
    for it in range(steps):
        inputs = _synthetic(states, variant)
        nxt = [ref.cell_fire_step(s, f, w, 0.01, 0.0, fx, wx, opts=opts) for s, (f, w, fx, wx) in zip(states, inputs)]
        if check:
            dev = _DeviceState(states)
            dev.step(np.concatenate([i[0] for i in inputs]), np.stack([i[1] for i in inputs]), 0.01, opts=opts,
                     extra=None if variant != 'extras' else np.concatenate([i[2] for i in inputs]),
                     virial_extra=None if variant != 'extras' else np.stack([i[3] for i in inputs]))
            _compare(dev, [n[0] for n in nxt], [n[1] for n in nxt])
        states = [n[0] for n in nxt]
        for _, w in nxt:
            seen['frozen' if w['branch'] is None else w['branch']] += 1
            seen['clipped'] += bool(w['clipped'])
            seen['guard'] += bool(w['guard'])
    return seen


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_kernel_follows_the_restatement_step_by_step(variant):
    seen = _kernel_sequence(variant)
    # both branches beyond the first step (every system starts uphill: v = 0), clipped moves, frozen systems, and no guard
    assert seen['uphill'] > len(SIZES) and seen['downhill'] > 0 and seen['clipped'] > 0 and seen['frozen'] > 0, seen
    assert seen['guard'] == 0, seen


def _moving_states(seed=3, sizes=(40, 300, 9)):
    rng = np.random.default_rng(seed)
    states = [ref.cell_fire_init(rng.normal(0, 1.0, (n, 3)), C0 @ F_INIT.T, cell0=C0) for n in sizes]
    for s in states:
        s['vel'] = rng.normal(0, 0.1, s['pos'].shape)
        s['vel_cell'] = rng.normal(0, 0.1, (3, 3))
        s['n_steps'], s['n_pos'], s['dt'], s['alpha'] = 4, 2, 0.07, 0.09
    return states, rng


def test_frozen_means_frozen():
    """an inactive system, and one whose generalised forces are already below fmax, keep pos, vel, cell and vel_cell bit for bit;
    the second is switched off with status 1 and no step counted; the third moves, cell included"""
    states, rng = _moving_states()
    states[0]['active'] = 0
    forces = [rng.normal(0, 5.0, (40, 3)), rng.normal(0, 1e-3, (300, 3)), rng.normal(0, 1.0, (9, 3))]
    virial = np.stack([rng.normal(0, 50.0, 6), rng.normal(0, 1e-3, 6), rng.normal(0, 5.0, 6)])
    dev = _DeviceState(states)
    pos0, vel0, cell0, vc0 = dev.pos.clone(), dev.vel.clone(), dev.cell.clone(), dev.vel_cell.clone()
    dev.step(np.concatenate(forces), virial, fmax=0.05)
    assert torch.equal(dev.pos[:340], pos0[:340]) and torch.equal(dev.vel[:340], vel0[:340])
    assert torch.equal(dev.cell[:2], cell0[:2]) and torch.equal(dev.vel_cell[:2], vc0[:2])
    assert not torch.equal(dev.pos[340:], pos0[340:]) and not torch.equal(dev.cell[2], cell0[2]) and not torch.equal(dev.vel_cell[2], vc0[2])
    assert torch.equal(dev.cell0, _t(np.stack([s['cell0'].reshape(9) for s in states]), torch.float64))   # read only
    assert dev.active.tolist() == [0, 0, 1] and dev.n_steps.tolist() == [4, 4, 5] and int(dev.n_active.item()) == 1
    assert dev.status.tolist() == [0, 1, 0]
    assert dev.dt.tolist()[:2] == [0.07, 0.07] and dev.alpha.tolist()[:2] == [0.09, 0.09] and dev.n_pos.tolist()[:2] == [2, 2]
    assert dev.fmax_sys[0].item() == -1.0 and 0 < dev.fmax_sys[1].item() < 0.05   # untouched / reported


def test_guard_refuses_an_inverted_and_a_flat_cell():
    """one launch of three systems of 4 atoms at F = I, the step unclipped (max_step 50) with dt = 0.05 after the first,
    uphill, step, so F_new = I + 0.0025 W / 16: the first virial inverts the cell (F_new = -0.56 I, det < 0); the third
    flattens z to 1 % (height 0.043 A under min_height = 5 / 64 A, det > 0); the second system moves.  The refused ones
    keep pos, cell and both velocities bit for bit with status 2, no step counted: a handled input, not a fault."""
    rng = np.random.default_rng(8)
    states = [ref.cell_fire_init(rng.random((4, 3)) @ C0, C0) for _ in range(3)]
    forces = [rng.normal(0, 0.5, (4, 3)).astype(np.float32) for _ in range(3)]
    virial = np.array([[-1e4, -1e4, -1e4, 0, 0, 0], [3.0, -2.0, 1.0, 0.5, -0.4, 0.2], [0, 0, -6336.0, 0, 0, 0]])
    min_h = 5.0 / 64
    nxt = [ref.cell_fire_step(s, f, w, 0.01, min_h, max_step=50.0) for s, f, w in zip(states, forces, virial)]
    what = [n[1] for n in nxt]
    assert [w['guard'] for w in what] == [True, False, True] and not what[1]['clipped']
    assert np.linalg.det(what[0]['F_new']) < 0                                                    # refused for the determinant
    assert np.linalg.det(what[2]['F_new']) > 0 and ref.min_height(C0 @ what[2]['F_new'].T) < min_h   # refused for the height
    dev = _DeviceState(states)
    pos0, cell0 = dev.pos.clone(), dev.cell.clone()
    dev.step(np.concatenate(forces), virial, 0.01, min_h, max_step=50.0)
    _compare(dev, [n[0] for n in nxt], what)
    assert dev.status.tolist() == [2, 0, 2] and dev.active.tolist() == [0, 1, 0] and dev.n_steps.tolist() == [0, 1, 0]
    assert int(dev.n_active.item()) == 1
    for b in (0, 2):
        assert torch.equal(dev.pos[4 * b:4 * b + 4], pos0[4 * b:4 * b + 4]) and torch.equal(dev.cell[b], cell0[b])
        assert not dev.vel[4 * b:4 * b + 4].any() and not dev.vel_cell[b].any()
    assert dev.dt.tolist() == [0.1, 0.05, 0.1] and dev.n_pos.tolist() == [0, 0, 0]
    assert not torch.equal(dev.pos[4:8], pos0[4:8]) and not torch.equal(dev.cell[1], cell0[1])
    # a non-finite virial is refused the same way
    dev = _DeviceState(states)
    virial[0, 1] = np.nan
    dev.step(np.concatenate(forces), virial, 0.01, min_h)
    assert dev.status.tolist() == [2, 0, 0] and torch.equal(dev.cell[0], cell0[0]) and torch.equal(dev.pos[:4], pos0[:4])


# ------------------------------------------------------------------------------------------------ the driver on an analytic energy
class _HarmonicForces:
    """the call interface and counters of batch.BatchForces over cellrelax_ref.harmonic_crystal, in fp64 torch on the device"""

    def __init__(self, systems):
        self.engine = SimpleNamespace(dev=torch.device(DEV))
        self.n_atoms = np.array([len(s['x0']) for s in systems], np.int64)
        self.x0 = [_t(s['x0'], torch.float64) for s in systems]
        self.metric0 = [_t(s['metric0'], torch.float64) for s in systems]
        self.n_force_calls = self.system_steps_evaluated = 0

    def __call__(self, pos, ids=None, want_atomic_virial=False, with_extra=True, cells_dev=None):
        ids = np.arange(len(self.n_atoms)) if ids is None else np.asarray(ids)
        sp = np.concatenate([[0], np.cumsum(self.n_atoms[ids])]).astype(np.int64)
        assert cells_dev.shape == (len(ids), 9) and pos.shape == (sp[-1], 3)
        parts = [ref.harmonic_crystal(pos[sp[k]:sp[k + 1]], cells_dev[k].reshape(3, 3), self.x0[b], self.metric0[b])
                 for k, b in enumerate(ids)]
        out = dict(forces=torch.cat([p[1] for p in parts]).float().contiguous(), energy_per_system=torch.stack([p[0] for p in parts]),
                   virial_per_system=torch.stack([torch.stack(ref.virial6(p[2])) for p in parts]).contiguous())
        self.n_force_calls += 1
        self.system_steps_evaluated += len(ids)
        return SimpleNamespace(seg_ptr=_t(sp, torch.int32), seg_ptr_host=sp), out, None, None


def _harmonic_systems():
    """four systems of 3 / 5 / 8 / 12 atoms: the start is the reference cell C0 (scaled per system) with rattled atoms, the
    minimum a cell strained by up to 4 % with the atoms on their sites"""
    rng = np.random.default_rng(21)
    out = []
    for n, scale in ((3, 1.0), (5, 1.1), (8, 0.95), (12, 1.2)):
        cell = scale * C0
        strain = rng.uniform(-0.04, 0.04, (3, 3))
        target = cell @ (np.eye(3) + 0.5 * (strain + strain.T))
        x0 = rng.random((n, 3))
        out.append(dict(x0=x0, metric0=target @ target.T, cell=cell, pos=x0 @ cell + rng.normal(0, 0.1, (n, 3))))
    return out


def _run_harmonic(systems, fmax=1e-4, steps=600, repack_below=0.0):
    from sevennet_amd.relax import check_cell_params, check_fire_params, fire_cell_loop
    forces = _HarmonicForces(systems)
    final, cells, n_steps, status, info = fire_cell_loop(
        forces, np.concatenate([s['pos'] for s in systems]), np.stack([s['cell'] for s in systems]), fmax=fmax, steps=steps,
        repack_below=repack_below, params=check_fire_params(fmax, steps, repack_below, {}),
        cell_params=check_cell_params(**ref.CELL), min_height=0.05)
    sp = np.concatenate([[0], np.cumsum(forces.n_atoms)])
    pos = final.cpu().numpy()
    return [dict(pos=pos[sp[b]:sp[b + 1]], cell=cells[b].cpu().numpy().reshape(3, 3), n_steps=int(n_steps[b]), status=int(status[b]))
            for b in range(len(systems))], info


@pytest.fixture(scope='module')
def harmonic():
    systems = _harmonic_systems()
    return SimpleNamespace(systems=systems, runs={rb: _run_harmonic(systems, repack_below=rb) for rb in (0.0, 1.0)})


def test_driver_finds_the_known_minimum(harmonic):
    """every generalised force row is below fmax when the kernel reports convergence; what that bounds, to first order around
    the minimum (the factor 1.5 covers the second order at these 1e-4-sized residuals): an atom's force f = g F^-1 is -k d, so
    |d| <= fmax |F^-1| / k; the cell force is G = W F^-T / n with W = -kappa C^T (C C^T - M) C - k sum d d^T, so
    |C C^T - M| <= (sqrt(3) n fmax |F| + k n max|d|^2) |C^-1|^2 / kappa (spectral norms, the three rows of G each below fmax)"""
    k, kappa, fmax = ref.HARMONIC['k'], ref.HARMONIC['kappa'], 1e-4
    res, info = harmonic.runs[0.0]
    for s, r in zip(harmonic.systems, res):
        n = len(s['x0'])
        assert r['status'] == 1 and 10 < r['n_steps'] < 600, r
        F = ref.deformation(r['cell'], s['cell'])
        nF, nFi, nCi = np.linalg.norm(F, 2), np.linalg.norm(np.linalg.inv(F), 2), np.linalg.norm(np.linalg.inv(r['cell']), 2)
        d_max = 1.5 * fmax * nFi / k
        d = np.sqrt(((r['pos'] - s['x0'] @ r['cell']) ** 2).sum(1)).max()
        m_max = 1.5 * (np.sqrt(3.0) * n * fmax * nF + k * n * d_max ** 2) * nCi ** 2 / kappa
        m = np.linalg.norm(r['cell'] @ r['cell'].T - s['metric0'], 2)
        print(f'n = {n}: {r["n_steps"]} steps, |d| {d:.2e} (bound {d_max:.2e}) A, |C C^T - M| {m:.2e} (bound {m_max:.2e}) A^2, '
              f'started at {np.linalg.norm(s["cell"] @ s["cell"].T - s["metric0"], 2):.2e}')
        assert d <= d_max and m <= m_max
        assert np.linalg.norm(s['cell'] @ s['cell'].T - s['metric0'], 2) > 10 * m_max   # (the start was nowhere near)
    assert info['n_repacks'] == 0 and info['fire_launches'] == max(r['n_steps'] for r in res) + 1
    assert info['n_force_calls'] == info['fire_launches'] and info['system_steps_evaluated'] == 4 * info['fire_launches']


def test_repacking_changes_nothing(harmonic):
    """a system's step depends on its own rows only (one workgroup per system, fixed summation order), so leaving the batch
    early changes no bit of anyone's result"""
    (res0, info0), (res1, info1) = harmonic.runs[0.0], harmonic.runs[1.0]
    assert info1['n_repacks'] > 0 and info0['n_repacks'] == 0
    assert info1['system_steps_evaluated'] < info0['system_steps_evaluated'] and info1['fire_launches'] == info0['fire_launches']
    for a, b in zip(res0, res1):
        assert (a['n_steps'], a['status']) == (b['n_steps'], b['status'])
        assert np.array_equal(a['pos'], b['pos']) and np.array_equal(a['cell'], b['cell'])


def test_a_system_alone_equals_itself_in_the_batch(harmonic):
    alone, info = _run_harmonic(harmonic.systems[2:3])
    a, b = alone[0], harmonic.runs[0.0][0][2]
    assert (a['n_steps'], a['status']) == (b['n_steps'], b['status']) and info['fire_launches'] == a['n_steps'] + 1
    assert np.array_equal(a['pos'], b['pos']) and np.array_equal(a['cell'], b['cell'])


# ------------------------------------------------------------------------------------------------ the driver on the model
def _strained(scale=1.0):
    D = np.eye(3) + scale * EPS
    return [(t, p @ D, c @ D, pbc) for t, p, c, pbc in _cells()]


@pytest.fixture(scope='module')
def model():
    from sevennet_amd.shapes import mini_sevennet_0_config
    calc, cfg, sd = _calc(mini_sevennet_0_config())
    return SimpleNamespace(calc=calc, cfg=cfg, sd=sd)


def _virial(res, cell):
    """the engine's virial (xx,yy,zz,xy,yz,zx) back from a results dict's stress"""
    return -res['stress'][[0, 1, 2, 5, 3, 4]] * abs(np.linalg.det(cell))


TRAJ_STEPS = 12
# |fp64 oracle - fp32 oracle| of the restatement after TRAJ_STEPS steps, per cell: positions and cell entries (A)
ORACLE_SPREAD = [(7.02e-9, 4.22e-9), (4.03e-9, 1.56e-9), (7.95e-9, 1.26e-9)]


def test_first_steps_follow_the_restatement_on_the_model(model):
    """12 steps on the device against the restatement driven by calc.compute_many on the host (all three cells in one call per
    step, as in the loop).  The bound is measured, not assumed: the restatement was run on the CPU with the fp64 oracle and with
    the fp32 oracle from the same start; after 12 steps the two differ by ORACLE_SPREAD (7.0e-9 / 4.0e-9 / 7.9e-9 A in the
    positions, 4.2e-9 / 1.6e-9 / 1.3e-9 A in the cell entries; the atoms moved 0.009 - 0.016 A, the cells 0.003 - 0.008 A).
    That is what single precision in the force call is worth over these steps; both sides here use the same fp32 engine, so
    they must agree within that spread times a margin of 10.  Needs the same P > 0 decisions, which are nowhere near a tie
    (cosine of g and v at least 0.999 from the second step on with the oracle; 0.5 is asserted)."""
    systems = _strained()
    numbers, pos, cells, pbcs = _args(systems)
    res = model.calc.relax_many(numbers, pos, cells, pbcs, fmax=FMAX, steps=TRAJ_STEPS, relax_cell=True)
    states = [ref.cell_fire_init(p, c) for p, c in zip(pos, cells)]
    cos = []
    for _ in range(TRAJ_STEPS):
        out = model.calc.compute_many(numbers, [s['pos'] for s in states], np.stack([s['cell'] for s in states]), pbcs)
        nxt = [ref.cell_fire_step(s, o['forces'], _virial(o, s['cell']), FMAX, model.calc.cutoff / 64) for s, o in zip(states, out)]
        states = [n[0] for n in nxt]
        cos.append(min(n[1]['cos'] for n in nxt))
    assert min(cos[1:]) > 0.5, cos
    for b, (s, r) in enumerate(zip(states, res)):
        assert s['n_steps'] == TRAJ_STEPS == r['n_steps'] and r['status'] == 'steps' and not r['converged']
        e_pos, e_cell = np.abs(r['positions'] - s['pos']).max(), np.abs(r['cell'] - s['cell']).max()
        print(f'cell {b}: max |dr| {e_pos:.3e} A (bound {10 * ORACLE_SPREAD[b][0]:.1e}), max |dC| {e_cell:.3e} A (bound '
              f'{10 * ORACLE_SPREAD[b][1]:.1e}), cell moved {np.abs(r["cell"] - cells[b]).max():.2e} A')
        assert e_pos <= 10 * ORACLE_SPREAD[b][0] and e_cell <= 10 * ORACLE_SPREAD[b][1], (b, e_pos, e_cell)
        assert np.abs(r['cell'] - cells[b]).max() > 1e-3   # (the cell did move)


def test_results_are_compute_many_at_the_returned_positions_and_cells(model):
    """energy, forces and stress of the results against compute_many there, within the batch-vs-single tolerances of
    test_batch_gpu.test_batch_equals_single_structure_calls; the stress uses the returned cell's volume"""
    systems = _strained()
    numbers, pos, cells, pbcs = _args(systems)
    res = model.calc.relax_many(numbers, pos, cells, pbcs, fmax=FMAX, steps=TRAJ_STEPS, relax_cell=True)
    info = model.calc.relax_info
    assert info['fire_launches'] == TRAJ_STEPS and info['n_force_calls'] == TRAJ_STEPS + 1 and info['n_repacks'] == 0
    many = model.calc.compute_many(numbers, [r['positions'] for r in res], np.stack([r['cell'] for r in res]), pbcs)
    for b, (r, m) in enumerate(zip(res, many)):
        assert abs(r['energy'] - m['energy']) <= 1e-6 * abs(m['energy']) + 1e-6, (b, r['energy'], m['energy'])
        assert np.abs(r['forces'] - m['forces']).max() <= 2e-5 * max(1.0, np.abs(m['forces']).max()), b
        assert np.abs(r['stress'] - m['stress']).max() <= 1e-5 * max(1e-3, np.abs(m['stress']).max()), b
        assert r['num_edges'] == m['num_edges']
        old = model.calc.compute_many(numbers[b:b + 1], [r['positions']], cells[b:b + 1], pbcs[b:b + 1])[0]   # at the caller's cell
        assert np.abs(r['stress'] - old['stress']).max() > 1e-5 * max(1e-3, np.abs(m['stress']).max()), b


def test_pressure_shrinks_the_cell(model):
    """0.05 eV/A^3 (8 GPa) against none, 12 steps each: with the fp64 oracle the volumes end at 150.4 / 150.0 / 315.6 A^3
    against 166.0 / 165.6 / 331.6"""
    numbers, pos, cells, pbcs = _args(_strained())
    free = model.calc.relax_many(numbers, pos, cells, pbcs, fmax=FMAX, steps=TRAJ_STEPS, relax_cell=True)
    pressed = model.calc.relax_many(numbers, pos, cells, pbcs, fmax=FMAX, steps=TRAJ_STEPS, relax_cell=True, scalar_pressure=0.05)
    for b, (f, p) in enumerate(zip(free, pressed)):
        vf, vp = abs(np.linalg.det(f['cell'])), abs(np.linalg.det(p['cell']))
        print(f'cell {b}: volume {vf:.2f} A^3 free, {vp:.2f} A^3 under pressure (start {abs(np.linalg.det(cells[b])):.2f})')
        assert vp < 0.97 * vf, (b, vp, vf)


def test_model_convergence(model):
    """The search described at the top found: strain EPS, no pressure, fmax 0.02 eV/A -- with the fp64 oracle all three cells
    converge without the guard tripping, after 50 / 31 / 43 moves (51 / 32 / 44 evaluations), at 0.888 / 0.977 / 1.011 of their
    starting volumes (at fmax 0.05 the first cell is converged where it starts).  Here: converged, the generalised forces of
    compute_many at the returned positions and cells below fmax + 1e-4 eV/A (the project's force-parity bar), energy below
    the initial one."""
    systems = _strained()
    numbers, pos, cells, pbcs = _args(systems)
    initial = model.calc.compute_many(numbers, pos, cells, pbcs)
    res = model.calc.relax_many(numbers, pos, cells, pbcs, fmax=FMAX, steps=200, relax_cell=True)
    info = model.calc.relax_info
    many = model.calc.compute_many(numbers, [r['positions'] for r in res], np.stack([r['cell'] for r in res]), pbcs)
    for b, (r, m) in enumerate(zip(res, many)):
        s = ref.cell_fire_init(r['positions'], r['cell'], cell0=cells[b])
        g = ref.generalised(s, m['forces'], _virial(m, r['cell']))[3]
        fm = np.sqrt((g * g).sum(1).max())
        print(f'cell {b}: {r["status"]} after {r["n_steps"]} moves, max generalised force {fm:.5f} eV/A, volume '
              f'{abs(np.linalg.det(r["cell"])) / abs(np.linalg.det(cells[b])):.4f} of the start, E {initial[b]["energy"]:.6f} -> {r["energy"]:.6f}')
        assert r['status'] == 'converged' and r['converged'] is True and 10 < r['n_steps'] < 200, (b, r['status'], r['n_steps'])
        assert fm < FMAX + 1e-4, (b, fm)
        assert r['energy'] < initial[b]['energy']
    assert info['fire_launches'] == max(r['n_steps'] for r in res) + 1 and info['n_force_calls'] == info['fire_launches'] + 1


class _Atoms:
    """what relax_many_atoms reads from and writes to an ASE Atoms"""

    def __init__(self, z, pos, cell, pbc):
        self.z, self.pos, self.cell, self.pbc = z, np.array(pos, float), np.array(cell, float), pbc

    def get_atomic_numbers(self):
        return np.asarray(self.z)

    def get_positions(self):
        return self.pos.copy()

    def get_cell(self):
        return self.cell.copy()

    def get_pbc(self):
        return np.asarray(self.pbc, bool)

    def set_positions(self, pos):
        self.pos = np.array(pos, float)

    def set_cell(self, cell, scale_atoms=True):
        assert scale_atoms is False
        self.cell = np.array(cell, float)


def test_surfaces(model):
    systems = _strained()
    numbers, pos, cells, pbcs = _args(systems)
    one = model.calc.compute(numbers[0], pos[0], cells[0], pbcs[0])
    res = model.calc.relax_many(numbers, pos, cells, pbcs, fmax=FMAX, steps=5, relax_cell=True, hydrostatic_strain=True)
    atoms = [_Atoms(z, p, c, pbc) for z, p, c, pbc in zip(numbers, pos, cells, pbcs)]
    via = model.calc.relax_many_atoms(atoms, fmax=FMAX, steps=5, relax_cell=True, hydrostatic_strain=True)
    for b, (r, v, a) in enumerate(zip(res, via, atoms)):
        assert set(r) == set(one) | {'positions', 'converged', 'n_steps', 'cell', 'status'} == set(v)
        assert r['cell'].shape == (3, 3) and r['cell'].dtype == np.float64 and r['status'] == 'steps' and r['converged'] is False
        assert np.array_equal(a.cell, v['cell']) and np.array_equal(a.pos, v['positions'])
        assert np.array_equal(v['cell'], r['cell']) and np.array_equal(v['positions'], r['positions'])
        lam = r['cell'][0, 0] / cells[b][0, 0]   # hydrostatic: a multiple of the caller's cell
        assert lam != 1.0 and np.abs(r['cell'] - lam * cells[b]).max() <= 1e-13 * np.abs(cells[b]).max()
    fixed = model.calc.relax_many(numbers, pos, cells, pbcs, fmax=FMAX, steps=5)   # today's keys without relax_cell
    assert set(fixed[0]) == set(one) | {'positions', 'converged', 'n_steps'}
    with pytest.raises(ValueError, match='system 1: relax_cell needs a cell periodic'):
        model.calc.relax_many(numbers[:2], pos[:2], cells[:2], np.array([[True] * 3, [True, False, True]]), relax_cell=True)
