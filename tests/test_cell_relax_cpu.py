"""CPU: variable-cell FIRE relaxation -- the fp64 restatement of the step (cellrelax_ref) pinned to the gradient of a periodic toy
pair potential and to the fixed-cell restatement, its projections, input validation before any device work, the device-cell
argument of the graph build and the adapter that writes the cell back.  The loop itself runs HIP kernels only and is covered on
the GPU (test_cell_relax_gpu.py)."""
import ctypes as C
import inspect
from types import SimpleNamespace

import numpy as np
import pytest

import cellrelax_ref as ref
import relax_ref
from test_relax_cpu import _NoDeviceEngine, _two_systems

RC = 3.0
C0 = np.array([[4.1, 0.0, 0.0], [0.7, 3.8, 0.0], [-0.5, 0.9, 4.3]])
F_INIT = np.array([[1.04, 0.03, -0.02], [0.01, 0.97, 0.05], [0.02, -0.04, 1.06]])


def toy(pos, cell):
    """a periodic pair potential phi(d) = (1 - d^2 / RC^2)^3 below RC, summed over pairs and images in fp64 -> (energy, forces
    [n,3], virial[6] in the engine's order xx,yy,zz,xy,yz,zx with its sign: virial = -dE/d(strain))"""
    n = len(pos)
    S = np.array([[a, b, c] for a in range(-2, 3) for b in range(-2, 3) for c in range(-2, 3)], np.float64) @ cell
    e, f, w = 0.0, np.zeros((n, 3)), np.zeros((3, 3))
    for i in range(n):
        for j in range(n):
            d = pos[j] - pos[i] + S
            d2 = (d * d).sum(1)
            m = (d2 < RC * RC) & (d2 > 1e-12)
            d, u = d[m], 1.0 - d2[m] / RC ** 2
            e += 0.5 * (u ** 3).sum()
            dphi = 0.5 * (3 * u ** 2 * (-2.0 / RC ** 2))[:, None] * d    # d(pair energy) / d(d vector), this ordered pair's half
            f[i] += dphi.sum(0)
            f[j] -= dphi.sum(0)
            w -= d.T @ dphi
    return e, f, np.array([w[0, 0], w[1, 1], w[2, 2], w[0, 1], w[1, 2], w[2, 0]])


def _state(n=5, seed=0, deformed=True):
    rng = np.random.default_rng(seed)
    cell = C0 @ F_INIT.T if deformed else C0.copy()
    pos = rng.random((n, 3)) @ cell
    return ref.cell_fire_init(pos, cell, cell0=C0)


def test_toy_potential_is_consistent():
    """forces and virial of the toy are the derivatives of its energy (central differences), so it can stand for a model"""
    s = _state()
    e, f, w = toy(s['pos'], s['cell'])
    h = 1e-5
    for i, k in ((0, 0), (3, 2)):
        dp = np.zeros_like(s['pos'])
        dp[i, k] = h
        num = -(toy(s['pos'] + dp, s['cell'])[0] - toy(s['pos'] - dp, s['cell'])[0]) / (2 * h)
        assert abs(num - f[i, k]) < 1e-7 * max(1.0, abs(f).max())
    W = ref.virial_matrix(w)
    assert np.array_equal(W, W.T)
    for a, b in ((0, 0), (1, 2)):
        eps = np.zeros((3, 3))
        eps[a, b] = eps[b, a] = h / 2 if a != b else h
        num = -(toy(s['pos'] @ (np.eye(3) + eps), s['cell'] @ (np.eye(3) + eps))[0]
                - toy(s['pos'] @ (np.eye(3) - eps), s['cell'] @ (np.eye(3) - eps))[0]) / (2 * h)
        assert abs(num - W[a, b]) < 1e-6 * abs(W).max()


@pytest.mark.parametrize('pressure', [0.0, 0.3])
def test_generalised_force_is_minus_the_gradient_of_the_enthalpy(pressure):
    """over all n + 3 rows of the coordinates (s_i; n F), with F != I and a triclinic C0: pins F, F^-T, the 1/n factor and the
    sign of the pressure.  Central differences with h = 1e-5 on a C^2 potential: error O(h^2 E''') ~ 1e-9, bound 1e-6 of the
    largest force component."""
    s = _state(n=6)
    n = len(s['pos'])
    _, f, w = toy(s['pos'], s['cell'])
    F, q, _, g = ref.generalised(s, f, w, scalar_pressure=pressure)
    assert np.linalg.cond(F) < 2 and np.abs(F - np.eye(3)).max() > 0.01

    def enthalpy(q):
        Fq = q[n:] / n
        cell = C0 @ Fq.T
        return toy(q[:n] @ Fq.T, cell)[0] + pressure * abs(np.linalg.det(cell))
    h = 1e-5
    num = np.zeros_like(q)
    for i in range(n + 3):
        for k in range(3):
            dq = np.zeros_like(q)
            dq[i, k] = h
            num[i, k] = -(enthalpy(q + dq) - enthalpy(q - dq)) / (2 * h)
    assert np.abs(num - g).max() < 1e-6 * np.abs(g).max(), (np.abs(num - g).max(), np.abs(g).max())
    assert np.abs(g[n:]).max() > 1e-3 and np.abs(g[:n]).max() > 1e-3   # (neither block is trivially zero)


def test_all_zero_mask_is_the_fixed_cell_step():
    """C = C0 and no strain component free: the trajectory of relax_ref.fire_step.  F = (C0^-1 C0)^T is I to a few ulp only and
    the positions go through r F^-T F_new^T each step, so equal means 1e-13 of the largest coordinate over 40 steps"""
    s = _state(deformed=False)
    fixed = relax_ref.fire_init(s['pos'])
    seen = set()
    for _ in range(40):
        _, f, w = toy(s['pos'], s['cell'])
        s, what = ref.cell_fire_step(s, f, w, 1e-3, opts=dict(cell_mask=[0] * 6))
        fixed, what0 = relax_ref.fire_step(fixed, toy(fixed['pos'], C0)[1], 1e-3)
        seen.add(what['branch'])
        assert what['branch'] == what0['branch'] and what['clipped'] == what0['clipped']
        assert (s['dt'], s['alpha'], s['n_pos'], s['n_steps']) == (fixed['dt'], fixed['alpha'], fixed['n_pos'], fixed['n_steps'])
        assert np.abs(s['pos'] - fixed['pos']).max() <= 1e-13 * np.abs(fixed['pos']).max()
        assert np.abs(s['vel'] - fixed['vel']).max() <= 1e-13 * max(np.abs(fixed['vel']).max(), 1e-300)
        assert not s['vel_cell'].any() and np.abs(s['cell'] - C0).max() <= 1e-14 * np.abs(C0).max()
    assert seen == {'uphill', 'downhill'}


def test_hydrostatic_strain_keeps_the_cell_a_multiple_of_the_reference():
    s = _state(deformed=False)
    for _ in range(25):
        _, f, w = toy(s['pos'], s['cell'])
        s, _ = ref.cell_fire_step(s, f, w, 1e-4, opts=dict(hydrostatic_strain=True, scalar_pressure=0.2))
    lam = s['cell'][0, 0] / C0[0, 0]
    assert abs(lam - 1.0) > 1e-3 and s['n_steps'] == 25
    assert np.abs(s['cell'] - lam * C0).max() <= 1e-13 * np.abs(C0).max()


def test_constant_volume_projects_the_trace_out():
    s = _state()
    n = len(s['pos'])
    _, f, w = toy(s['pos'], s['cell'])
    g_free = ref.generalised(s, f, w, scalar_pressure=0.1)[3]
    g = ref.generalised(s, f, w, scalar_pressure=0.1, constant_volume=True)[3]
    assert abs(np.trace(g_free[n:])) > 1e-3
    assert abs(np.trace(g[n:])) <= 1e-15 * np.abs(g_free[n:]).max() * 3
    off = ~np.eye(3, dtype=bool)
    assert np.array_equal(g[n:][off], g_free[n:][off]) and np.array_equal(g[:n], g_free[:n])
    # the mask comes before the projection: a masked diagonal entry still gets its share of the trace taken off
    g = ref.generalised(s, f, w, constant_volume=True, cell_mask=[1, 1, 0, 1, 1, 1])[3][n:]
    assert abs(np.trace(g)) <= 1e-15 * np.abs(g_free[n:]).max() * 3 and g[2, 2] != 0.0


def test_guard_of_the_restatement():
    s = _state()
    _, f, w = toy(s['pos'], s['cell'])
    big = np.array([-1e6, -1e6, -1e6, 0, 0, 0.0])
    nxt, what = ref.cell_fire_step(s, f, big, 1e-3, min_h=0.0)
    assert what['clipped'] and nxt['status'] == 0      # a step clipped to 0.2 moves F by 0.2 / n at most: no inversion from near I
    nxt, what = ref.cell_fire_step(s, f, big, 1e-3, min_h=0.0, max_step=5000.0)
    assert what['guard'] and nxt['status'] == 2 and nxt['active'] == 0 and nxt['n_steps'] == 0   # an unclipped one inverts it
    assert np.linalg.det(what['F_new']) < 0
    for k in ('pos', 'vel', 'cell', 'vel_cell'):
        assert np.array_equal(nxt[k], s[k])
    assert (nxt['dt'], nxt['alpha'], nxt['n_pos']) == (s['dt'], s['alpha'], s['n_pos'])
    nxt, what = ref.cell_fire_step(s, f, w, 1e-3, min_h=10.0)   # no height of this cell reaches 10 A
    assert what['guard'] and nxt['status'] == 2
    assert ref.min_height(np.diag([2.0, 3.0, 4.0])) == pytest.approx(2.0, rel=1e-15)


def test_harmonic_crystal_is_consistent_and_rotation_invariant():
    """the analytic energy that drives the loop on the GPU: forces and virial are its derivatives, the virial is symmetric, a
    common rotation of atoms and cell changes nothing, and it vanishes with its forces at the stated minimum"""
    rng = np.random.default_rng(4)
    s = _state(n=4)
    x0 = rng.random((4, 3))
    target = C0 @ (np.eye(3) + 0.03 * np.array([[1.0, 0.3, 0], [0.3, -1, 0.2], [0, 0.2, 0.5]]))
    m0 = target @ target.T
    e, f, W = ref.harmonic_crystal(s['pos'], s['cell'], x0, m0)
    assert np.abs(W - W.T).max() <= 1e-15 * np.abs(W).max()
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    e_rot = ref.harmonic_crystal(s['pos'] @ q, s['cell'] @ q, x0, m0)[0]
    assert abs(e_rot - e) <= 1e-13 * e
    h = 1e-5
    for a, b in ((0, 0), (1, 2), (2, 2)):
        eps = np.zeros((3, 3))
        eps[a, b] = eps[b, a] = h / 2 if a != b else h
        num = -(ref.harmonic_crystal(s['pos'] @ (np.eye(3) + eps), s['cell'] @ (np.eye(3) + eps), x0, m0)[0]
                - ref.harmonic_crystal(s['pos'] @ (np.eye(3) - eps), s['cell'] @ (np.eye(3) - eps), x0, m0)[0]) / (2 * h)
        assert abs(num - W[a, b]) <= 1e-7 * np.abs(W).max()
    dp = np.zeros((4, 3))
    dp[2, 1] = h
    num = -(ref.harmonic_crystal(s['pos'] + dp, s['cell'], x0, m0)[0] - ref.harmonic_crystal(s['pos'] - dp, s['cell'], x0, m0)[0]) / (2 * h)
    assert abs(num - f[2, 1]) <= 1e-7 * np.abs(f).max()
    e, f, W = ref.harmonic_crystal(x0 @ target, target, x0, m0)
    assert e == 0.0 and not f.any() and not W.any()


# ------------------------------------------------------------------------------------------------ validation
def _relax(**kw):
    from sevennet_amd.relax import relax_batch
    types, pos, cells, pbcs = _two_systems()
    cells, pbcs = np.stack([np.eye(3) * 6.0] * 2), np.ones((2, 3), bool)
    args = dict(types=types, positions=pos, cells=cells, pbcs=pbcs, cutoff=5.0, relax_cell=True)
    args.update(kw)
    return relax_batch(_NoDeviceEngine(), args.pop('types'), args.pop('positions'), args.pop('cells'), args.pop('pbcs'), **args)


@pytest.mark.parametrize('kw, match', [
    (dict(cell_mask=[1, 1, 1]), 'cell_mask'),
    (dict(cell_mask=[1, 1, 1, 0, 0, 2]), 'cell_mask'),
    (dict(cell_mask=[1, 1, 1, 0, 0, 0.5]), 'cell_mask'),
    (dict(cell_mask=np.ones((3, 3))), 'cell_mask'),
    (dict(scalar_pressure=float('nan')), 'scalar_pressure'),
    (dict(scalar_pressure=float('inf')), 'scalar_pressure'),
    (dict(scalar_pressure='high'), 'scalar_pressure'),
    (dict(hydrostatic_strain=True, constant_volume=True), 'hydrostatic_strain and constant_volume'),
    (dict(extra=lambda *a: None), 'no virial'),
    (dict(pbcs=np.array([[True] * 3, [True, True, False]])), 'system 1: relax_cell needs a cell periodic'),
    (dict(cells=np.stack([np.eye(3) * 6.0, np.diag([6.0, 6.0, 0.05])])), 'system 1: .*height below cutoff / 64'),
    (dict(relax_cel=True), 'unknown FIRE parameter'),
])
def test_bad_cell_arguments_raise_before_any_device_work(kw, match):
    with pytest.raises(ValueError, match=match):
        _relax(**kw)


def test_cell_arguments_are_checked_without_relax_cell_too_and_d3_refuses():
    with pytest.raises(ValueError, match='cell_mask'):
        _relax(relax_cell=False, cell_mask=[1])
    from sevennet_amd.d3 import SevenNetD3Calculator
    calc = object.__new__(SevenNetD3Calculator)   # (refused before the calculator's engines are looked at)
    with pytest.raises(ValueError, match='no virial'):
        calc.relax_many([[14]], [np.zeros((1, 3))], np.eye(3)[None] * 6.0, [True] * 3, relax_cell=True)


def test_too_many_atoms_for_the_batched_kernel_names_the_system():
    from sevennet_amd.batch import BATCH_MAX_ATOMS
    from sevennet_amd.relax import check_cell_relax_systems
    cells, pbcs = np.stack([np.eye(3) * 6.0] * 2), np.ones((2, 3), bool)
    check_cell_relax_systems([4, BATCH_MAX_ATOMS], cells, pbcs, 5.0)
    with pytest.raises(ValueError, match='system 1: .*more atoms'):
        check_cell_relax_systems([4, BATCH_MAX_ATOMS + 1], cells, pbcs, 5.0)


def test_cell_params():
    from sevennet_amd.relax import STATUS_NAMES, check_cell_params
    assert check_cell_params(0.0, None, False, False) == dict(scalar_pressure=0.0, cell_mask_bits=63, hydrostatic_strain=False,
                                                              constant_volume=False)
    p = check_cell_params(np.float32(0.5), (1, 0, 0, 0, 1, 0), 1, 0)
    assert p == dict(scalar_pressure=0.5, cell_mask_bits=0b010001, hydrostatic_strain=True, constant_volume=False)
    assert check_cell_params(0, np.array([True, False, True, False, False, True]), False, True)['cell_mask_bits'] == 0b100101
    assert STATUS_NAMES == ('steps', 'converged', 'cell_failed')
    from sevennet_amd import _lib
    assert len(_lib.SIGNATURES['snet_fire_cell_step'][1]) == 35 and len(_lib.SIGNATURES['snet_fire_step'][1]) == 24


# ------------------------------------------------------------------------------------------------ the device-cell argument
def test_device_cell_argument_defaults_to_the_host_path(monkeypatch):
    """cells_dev defaults to None everywhere, and with None the neighbor kernels get an upload of the host cells: a stand-in
    library records the cells it is handed (the count kernel's stand-in reports no edges, so nothing else is launched)"""
    import torch
    from sevennet_amd import _lib, batch
    for fn in (batch._batched_neighbors, batch.build_batch_graph, batch.BatchForces.__call__):
        assert inspect.signature(fn).parameters['cells_dev'].default is None
    seen = []

    def count(pos, ap, B, cells, pbc, n, cutoff, count, st):
        seen.append(np.ctypeslib.as_array(C.cast(cells, C.POINTER(C.c_double)), (B * 9,)).copy())
        C.memset(count, 0, 4 * n)
        return 0
    monkeypatch.setattr(_lib, 'load', lambda: SimpleNamespace(snet_batch_nl_count=count))
    monkeypatch.setattr(_lib, 'stream', lambda: None)
    cells = np.stack([C0, 2.0 * C0])
    pos = torch.zeros(5, 3, dtype=torch.float64)
    out = batch._batched_neighbors(pos, np.array([0, 2, 5]), cells, np.ones((2, 3), bool), RC, 'cpu', False)
    assert out[-1] == 0 and len(seen) == 1 and np.array_equal(seen[0], cells.reshape(-1))
    with pytest.raises(ValueError, match='cells_dev'):   # a tensor that is not on the GPU is refused, not copied
        batch._batched_neighbors(pos, np.array([0, 2, 5]), cells, np.ones((2, 3), bool), RC, 'cpu', False,
                                 cells_dev=torch.zeros(2, 9, dtype=torch.float64))
    assert len(seen) == 1


# ------------------------------------------------------------------------------------------------ bookkeeping and adapters
def test_repack_book_keeps_cells_and_status():
    from sevennet_amd.relax import RepackBook
    book = RepackBook(np.array([2, 1, 3]))
    pos = np.arange(18.0).reshape(6, 3)
    cells = np.arange(27.0).reshape(3, 9)
    keep, rows = book.repack(pos, np.array([1, 0, 0]), np.array([3, 2, 3]), cells=cells, status=np.array([0, 1, 2]))
    assert keep.tolist() == [0] and rows.tolist() == [0, 1]
    book.store(pos[rows] + 1.0, np.array([1]), np.array([7]), only_finished=False, cells=cells[keep] + 1.0, status=np.array([0]))
    assert book.status.tolist() == [0, 1, 2] and book.converged.tolist() == [False, True, False] and book.n_steps.tolist() == [7, 2, 3]
    assert np.array_equal(np.stack(book.cells), cells + np.array([1.0, 0, 0])[:, None])
    plain = RepackBook(np.array([1, 1]))   # without cells the fixed-cell meaning of converged stays
    plain.store(pos[:2], np.array([0, 1]), np.array([1, 1]), only_finished=False)
    assert plain.converged.tolist() == [True, False] and plain.cells == [None, None]


class _Atoms:
    def __init__(self):
        self.log = []

    def get_atomic_numbers(self):
        return np.array([14, 14])

    def get_positions(self):
        return np.zeros((2, 3))

    def get_cell(self):
        return np.eye(3) * 5.0

    def get_pbc(self):
        return np.ones(3, bool)

    def set_cell(self, cell, scale_atoms=True):
        self.log.append(('cell', np.array(cell), scale_atoms))

    def set_positions(self, pos):
        self.log.append(('positions', np.array(pos)))


def test_atoms_adapter_writes_the_cell_back_before_the_positions():
    from sevennet_amd.atoms import ManyAtomsMixin

    class Host(ManyAtomsMixin):
        def relax_many(self, numbers, positions, cells, pbcs, **kw):
            self.kw = kw
            return [{'positions': np.full((2, 3), b + 1.0), 'cell': np.eye(3) * (6.0 + b)} for b in range(len(numbers))]
    host, atoms = Host(), [_Atoms(), _Atoms()]
    host.relax_many_atoms(atoms, fmax=0.01, steps=9, relax_cell=True, scalar_pressure=0.1)
    assert host.kw == dict(fmax=0.01, steps=9, relax_cell=True, scalar_pressure=0.1)
    for b, a in enumerate(atoms):
        assert [e[0] for e in a.log] == ['cell', 'positions'] and a.log[0][2] is False
        assert np.array_equal(a.log[0][1], np.eye(3) * (6.0 + b)) and np.array_equal(a.log[1][1], np.full((2, 3), b + 1.0))
    atoms = [_Atoms()]
    host.relax_many_atoms(atoms, relax_cell=False)    # at fixed cells the cell is not touched
    assert [e[0] for e in atoms[0].log] == ['positions']
