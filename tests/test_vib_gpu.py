"""GPU: batched finite-difference Hessians -- the three kernels against their fp64 restatement (vib_ref), the loop on a
potential whose Hessian is known, and the driver and the public surfaces on a model: the 15-atom vacancy cell of the band tests
with five atoms displaced, a five-atom molecule without a cell and one isolated atom, against vib_ref driven by the fp64 oracle
at the same displacements."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vib_ref
from helpers import oracle_model
from test_batch_gpu import Z, _calc, _systems
from test_neb_gpu import model_bands
from test_relax_gpu import D3_CUT, DEV, _Atoms, _oracle

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
DELTA = 0.01


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


# ------------------------------------------------------------------------------------------------ the kernels
KERNEL_N = [1, 5, 300, 64]   # 300: more atoms than threads; 64: a quarter of the atoms selected, not in order


def _kernel_case(nfree):
    """every copy of four systems in one call, with random fp32 forces and fp64 extra forces on them"""
    from sevennet_amd.vib import plan_copies
    rng = np.random.default_rng(11)
    sel = [np.arange(1), np.arange(5), np.arange(300), rng.permutation(64)[:16]]
    plan = plan_copies(KERNEL_N, sel, nfree, 10 ** 7)
    assert len(plan.calls) == 1
    call = plan.calls[0]
    n = np.array(KERNEL_N)
    pos0 = [rng.uniform(-3.0, 9.0, (k, 3)) for k in KERNEL_N]
    copy_ptr = np.concatenate([[0], np.cumsum(n[call.desc[:, 0]])])
    N = int(copy_ptr[-1])
    return SimpleNamespace(nfree=nfree, sel=sel, call=call, n=n, pos0=pos0, copy_ptr=copy_ptr, N=N,
                           f32=rng.normal(0.0, 1.0, (N, 3)).astype(np.float32), fx=rng.normal(0.0, 1e-2, (N, 3)),
                           masses=[rng.uniform(1.0, 60.0, k) for k in KERNEL_N])


def _displace(case, desc=None, copy_ptr=None):
    from sevennet_amd.vib import vib_displace
    desc = case.call.desc if desc is None else desc
    copy_ptr = case.copy_ptr if copy_ptr is None else copy_ptr
    pos = torch.full((case.N, 3), 123.0, dtype=torch.float64, device=DEV)
    status = torch.zeros(len(desc), dtype=torch.int32, device=DEV)
    vib_displace(_t(np.concatenate(case.pos0), torch.float64), _t(np.concatenate([[0], np.cumsum(case.n)]), torch.int32),
                 _t(desc, torch.int32), _t(copy_ptr, torch.int32), DELTA, pos, status)
    torch.cuda.synchronize()
    return pos.cpu().numpy(), status.cpu().numpy()


def _reduce(case, f32=None):
    """snet_vib_rows + snet_vib_finish on the case's forces -> (D, H, Hm per system, asymmetry, status)"""
    from sevennet_amd.vib import vib_finish, vib_rows
    m = np.array([len(s) for s in case.sel])
    d_off = np.concatenate([[0], np.cumsum(9 * m * m)])
    f64, i32 = torch.float64, torch.int32
    D = torch.full((int(d_off[-1]),), 7.0, dtype=f64, device=DEV)   # (rows are written, not accumulated: the 7.0 must go)
    status = torch.zeros(4, dtype=i32, device=DEV)
    sel_ptr, off_d = _t(np.concatenate([[0], np.cumsum(m)]), i32), _t(d_off[:-1], torch.int64)
    vib_rows(_t(case.f32 if f32 is None else f32, torch.float32), _t(case.fx, f64), _t(case.copy_ptr, i32), _t(case.call.groups, i32),
             case.nfree, DELTA, _t(np.concatenate(case.sel), i32), sel_ptr, off_d, D, status)
    H, Hm, asym = torch.empty_like(D), torch.empty_like(D), torch.empty(4, dtype=f64, device=DEV)
    w = np.concatenate([1.0 / np.sqrt(ms[s]) for ms, s in zip(case.masses, case.sel)])
    vib_finish(D, off_d, sel_ptr, _t(w, f64), status, H, Hm, asym)
    torch.cuda.synchronize()
    cut = lambda a: [a.cpu().numpy()[d_off[b]:d_off[b + 1]].reshape(3 * m[b], 3 * m[b]) for b in range(4)]   # noqa: E731
    return cut(D), cut(H), cut(Hm), asym.cpu().numpy(), status.cpu().numpy()


def _restated(case):
    """vib_ref on the bits the kernels see: fp32 forces widened plus the fp64 ones -> per system (D, scale, H, Hm, asymmetry)"""
    F = case.f32.astype(np.float64) + case.fx
    out = []
    for b in range(4):
        m3 = 3 * len(case.sel[b])
        D, scale = np.zeros((m3, m3)), np.zeros((m3, m3))
        for j0, gb, r in case.call.groups:
            if gb != b:
                continue
            rows = [F[case.copy_ptr[j0 + w]:case.copy_ptr[j0 + w + 1]][case.sel[b]].reshape(-1) for w in range(case.nfree)]
            D[r] = vib_ref.row(rows, case.nfree, DELTA)
            scale[r] = sum(wt * np.abs(f) for wt, f in zip(vib_ref.WEIGHTS[case.nfree], rows)) / DELTA
        out.append((D, scale) + vib_ref.finish(D, case.masses[b][case.sel[b]]))
    return out


@pytest.mark.parametrize('nfree', [2, 4])
def test_kernels_equal_the_restatement(nfree):
    """pos_out bit for bit; every element of D within 8 x 2^-53 x sum_w |weight_w F_w| / delta (at most 8 roundings: the extra
    force added, the products by 8, three sums and the division), H within the same bound and bitwise symmetric, the asymmetry
    equal to the restatement's"""
    case = _kernel_case(nfree)
    pos, status = _displace(case)
    assert not status.any()
    want = np.concatenate([vib_ref.displaced(case.pos0[b], a, i, q, DELTA) for b, a, i, q in case.call.desc.tolist()])
    assert np.array_equal(pos, want)
    moved = sum(int((pos[case.copy_ptr[j]:case.copy_ptr[j + 1]] != case.pos0[d[0]]).sum()) for j, d in enumerate(case.call.desc.tolist()))
    assert moved == len(case.call.desc) - 4   # one component per displaced copy, none of the four undisplaced ones
    D, H, Hm, asym, status = _reduce(case)
    assert not status.any()
    for b, (D_ref, scale, H_ref, Hm_ref, asym_ref) in enumerate(_restated(case)):
        tol = 8 * EPS * scale
        print(f'nfree {nfree}, system {b} (n {KERNEL_N[b]}, m {len(case.sel[b])}): max |dD| {np.abs(D[b] - D_ref).max():.3e}, max |dH| '
              f'{np.abs(H[b] - H_ref).max():.3e} (smallest bound {tol.min():.3e}), asymmetry {asym[b]:.6e} (restatement {asym_ref:.6e})')
        assert (np.abs(D[b] - D_ref) <= tol).all()
        assert (np.abs(H[b] - H_ref) <= np.maximum(tol, tol.T)).all()
        assert np.array_equal(H[b], H[b].T) and np.array_equal(Hm[b], Hm[b].T)
        w = np.repeat(1.0 / np.sqrt(case.masses[b][case.sel[b]]), 3)
        assert np.array_equal(Hm[b], H[b] * (w[:, None] * w[None, :]))
        assert asym[b] == asym_ref


def test_a_descriptor_that_does_not_fit_is_refused_and_its_rows_are_left_alone():
    case = _kernel_case(2)
    ref, _ = _displace(case)
    desc = case.call.desc.copy()
    first = {b: int(np.nonzero(desc[:, 0] == b)[0][0]) for b in range(4)}
    wrong_span, wrong_atom, wrong_axis, wrong_system = first[1] + 2, first[3] + 5, first[1] + 4, first[0]
    desc[wrong_span, 0] = 3          # a 5-row copy described as a copy of the 64-atom system
    desc[wrong_atom, 1] = 64         # one past the last atom
    desc[wrong_axis, 2] = 3
    desc[wrong_system, 0] = 4
    pos, status = _displace(case, desc=desc)
    bad = [wrong_span, wrong_atom, wrong_axis, wrong_system]
    assert np.nonzero(status)[0].tolist() == sorted(bad) and set(status[bad].tolist()) == {1}
    for j in range(len(desc)):
        rows = slice(case.copy_ptr[j], case.copy_ptr[j + 1])
        if j in bad:
            assert (pos[rows] == 123.0).all()
        else:
            assert np.array_equal(pos[rows], ref[rows])


def test_a_force_that_is_not_finite_fails_its_system_alone():
    case = _kernel_case(2)
    _, H0, Hm0, asym0, _ = _reduce(case)
    f32 = case.f32.copy()
    j0 = int(case.call.groups[np.nonzero(case.call.groups[:, 1] == 1)[0][3], 0])   # a displaced copy of system 1
    f32[case.copy_ptr[j0] + 2, 1] = np.inf
    _, H, Hm, asym, status = _reduce(case, f32=f32)
    assert status.tolist() == [0, 2, 0, 0]
    assert np.isnan(H[1]).all() and np.isnan(Hm[1]).all() and np.isnan(asym[1])
    for b in (0, 2, 3):
        assert np.array_equal(H[b], H0[b]) and np.array_equal(Hm[b], Hm0[b]) and asym[b] == asym0[b]


# ------------------------------------------------------------------------------------------------ the loop, analytic potential
class _QuadraticForces:
    """E = (x - x0)^T K (x - x0) / 2 per system in torch on the device, behind the call interface of batch.BatchForces over
    the copy slots of a plan: the fp32 forces are zero, the fp64 forces go through the extra slot.  Each copy is one
    matrix-vector product of its own, so a copy's forces do not depend on what else is in the call."""

    def __init__(self, slot_system, K, x0):
        self.slot_system = np.asarray(slot_system, np.int64)
        self.K = [_t(k, torch.float64) for k in K]
        self.x0 = [_t(np.asarray(x).reshape(-1), torch.float64) for x in x0]
        self.n = np.array([len(x) for x in x0], np.int64)
        self.engine = SimpleNamespace(dev=torch.device(DEV))
        self.n_force_calls = 0

    def __call__(self, pos, ids=None, **kw):
        systems = self.slot_system[np.asarray(ids, np.int64)]
        seg = np.concatenate([[0], np.cumsum(self.n[systems])])
        f = torch.cat([-torch.mv(self.K[b], pos[int(seg[j]):int(seg[j + 1])].reshape(-1) - self.x0[b]) for j, b in enumerate(systems)])
        self.n_force_calls += 1
        g = SimpleNamespace(seg_ptr=_t(seg, torch.int32), seg_ptr_host=seg)
        out = dict(forces=torch.zeros(len(pos), 3, dtype=torch.float32, device=pos.device),
                   energy_per_system=torch.zeros(len(systems), dtype=torch.float64, device=pos.device))
        return g, out, f.reshape(-1, 3).contiguous(), torch.zeros(len(systems), dtype=torch.float64, device=pos.device)


def _quadratic_systems():
    rng = np.random.default_rng(4)
    n = [1, 5, 7]
    sel = [np.arange(1), np.arange(5), np.array([6, 0, 3])]
    K = [vib_ref.random_spd_like(rng, 3 * k) for k in n]
    x0 = [rng.normal(0.0, 1.0, (k, 3)) for k in n]
    pos = [x + rng.normal(0.0, 0.3, x.shape) for x in x0]
    masses = [rng.uniform(1.0, 30.0, k) for k in n]
    return n, sel, K, x0, pos, masses


def _quadratic_loop(which, nfree, budget):
    from sevennet_amd.vib import plan_copies, vib_loop
    n, sel, K, x0, pos, masses = ([a[b] for b in which] for a in _quadratic_systems())
    plan = plan_copies(n, sel, nfree, budget)
    forces = _QuadraticForces(plan.slot_system, K, x0)
    H, Hm, asym, status, info = vib_loop(forces, plan, np.concatenate(pos), n, sel, masses, delta=DELTA)
    return H, Hm, asym, status, info, plan


@pytest.mark.parametrize('nfree', [2, 4])
def test_loop_recovers_a_known_hessian_whatever_the_packing(nfree):
    n, sel, K, x0, pos, masses = _quadratic_systems()
    H, Hm, asym, status, info, plan = _quadratic_loop([0, 1, 2], nfree, 10 ** 6)
    assert len(plan.calls) == 1 and status.tolist() == [0, 0, 0]
    for b in range(3):
        rows = (3 * sel[b][:, None] + np.arange(3)).reshape(-1)
        force = vib_ref.quadratic(K[b], x0[b])
        fmax = max(np.abs(force(vib_ref.displaced(pos[b], a, i, q, DELTA))).max() for a in sel[b] for i in range(3) for q in (-2, 2))
        err, tol = np.abs(H[b] - K[b][np.ix_(rows, rows)]).max(), 16 * EPS * fmax / DELTA   # the bound of test_vib_cpu
        print(f'nfree {nfree}, system {b}: max |H - K| {err:.3e} (bound {tol:.3e}), asymmetry {asym[b]:.3e}')
        assert err <= tol
        w = np.repeat(1.0 / np.sqrt(masses[b][sel[b]]), 3)
        assert np.array_equal(Hm[b], H[b] * (w[:, None] * w[None, :]))
    copies = sum(nfree * 3 * len(s) + 1 for s in sel)
    assert info['n_force_calls'] == 1 and info['copies_evaluated'] == copies and info['launches'] == 3
    # one item per call: the same bits
    H1, Hm1, asym1, _, info1, plan1 = _quadratic_loop([0, 1, 2], nfree, 1)
    assert len(plan1.calls) == sum(3 * len(s) + 1 for s in sel) and all(len(c.groups) + len(c.base) == 1 for c in plan1.calls)
    assert info1['n_force_calls'] == len(plan1.calls) and info1['copies_evaluated'] == copies
    # a budget between the two
    H2, _, _, _, info2, plan2 = _quadratic_loop([0, 1, 2], nfree, 60)
    assert 1 < len(plan2.calls) < len(plan1.calls) and info2['n_force_calls'] == len(plan2.calls)
    for b in range(3):
        assert np.array_equal(H1[b], H[b]) and np.array_equal(Hm1[b], Hm[b]) and asym1[b] == asym[b] and np.array_equal(H2[b], H[b])
    # a system alone: the same bits as inside the batch
    Ha, Hma, asyma, _, infoa, _ = _quadratic_loop([1], nfree, 10 ** 6)
    assert np.array_equal(Ha[0], H[1]) and np.array_equal(Hma[0], Hm[1]) and asyma[0] == asym[1]
    assert infoa['copies_evaluated'] == nfree * 15 + 1


# ------------------------------------------------------------------------------------------------ the driver on a model
MASS = {14: 28.0855, 8: 15.999, 6: 12.011, 1: 1.008}
F_TOL = 1e-4   # the force tolerance of test_batch_gpu.test_batch_against_the_fp64_oracle for this engine (eV/A)
SUBSET = np.array([0, 3, 7, 11, 14])   # of the 15-atom cell: the hopping atom and four others


def model_systems():
    """[(types, positions, cell, pbc, indices)]: the initial image of the first vacancy band (15 atoms, five displaced), the
    molecule of the batch tests (all atoms) and one isolated atom"""
    bands = model_bands()
    types, images, cell, pbc = bands[0]
    out = [(types, images[0], cell, pbc, SUBSET)]
    types, images, cell, pbc = bands[2]
    out.append((types, images[0], cell, pbc, None))
    types, pos, cell, pbc = _systems(2)[5]
    out.append((types, pos, cell, pbc, None))
    return out


def _vib_args(systems):
    numbers = [np.array(Z)[s[0]] for s in systems]
    return (numbers, [s[1] for s in systems], [np.array([MASS[z] for z in zs]) for zs in numbers], np.stack([s[2] for s in systems]),
            np.array([s[3] for s in systems]))


@pytest.fixture(scope='module')
def model():
    from sevennet_amd.shapes import mini_sevennet_0_config
    calc, cfg, sd = _calc(mini_sevennet_0_config())
    return SimpleNamespace(calc=calc, cfg=cfg, sd=sd, orc=oracle_model(cfg, sd))


@pytest.fixture(scope='module')
def runs(model):
    """vibrations_many for both nfree, once"""
    systems = model_systems()
    out = {}
    for nfree in (2, 4):
        res = model.calc.vibrations_many(*_vib_args(systems), delta=DELTA, nfree=nfree, indices=[s[4] for s in systems])
        out[nfree] = (res, dict(model.calc.vib_info))
    return systems, out


@pytest.mark.parametrize('nfree', [2, 4])
def test_hessians_against_the_fp64_oracle(model, runs, nfree):
    """|dH| <= c f_tol / delta, c = 1 (nfree 2) or 1.5 (nfree 4): the sums of the stencil weights times the engine's force
    tolerance; |d lambda| <= 3m max |dHm| (Weyl, with the Frobenius norm above the spectral norm).  Eigenvalues, not
    frequencies: the square root is unbounded near zero."""
    systems, out = runs
    res, info = out[nfree]
    c = {2: 1.0, 4: 1.5}[nfree]
    args = _vib_args(systems)
    assert info['copies_evaluated'] == sum(nfree * 3 * (len(s[0]) if s[4] is None else len(s[4])) + 1 for s in systems)
    assert info['n_force_calls'] == 1 and info['launches'] == 3   # everything fits one call
    for b, (types, pos, cell, pbc, idx) in enumerate(systems):
        ref = vib_ref.vibrations(lambda p: _oracle(model, types, p, cell, pbc)[1], pos, args[2][b], idx, DELTA, nfree)
        r = res[b]
        m = len(ref['eigenvalues']) // 3
        err, tol = np.abs(r['hessian'] - ref['hessian']).max(), c * F_TOL / DELTA
        w = np.repeat(1.0 / np.sqrt(args[2][b][r['indices']]), 3)
        d_hm = np.abs(r['hessian'] * (w[:, None] * w[None, :]) - ref['hessian_mw']).max()
        d_lam = np.abs(r['eigenvalues'] - ref['eigenvalues']).max()
        print(f'nfree {nfree}, system {b} (m {m}): max |dH| {err:.3e} eV/A^2 (bound {tol:.3e}), max |d lambda| {d_lam:.3e} (bound '
              f'{3 * m * d_hm:.3e}), asymmetry {r["asymmetry"]:.3e} (oracle {ref["asymmetry"]:.3e}), max |H| {np.abs(ref["hessian"]).max():.3e}')
        assert r['status'] == 'ok' and np.array_equal(r['indices'], np.arange(len(types)) if idx is None else idx)
        assert err <= tol
        assert d_lam <= 3 * m * d_hm
        assert np.array_equal(r['hessian'], r['hessian'].T) and r['hessian'].shape == (3 * m, 3 * m)
        modes = r['modes'].reshape(3 * m, 3 * m)
        assert r['modes'].shape == (3 * m, m, 3) and np.abs(modes @ modes.T - np.eye(3 * m)).max() <= 1e-12
        assert np.array_equal(r['frequencies'], r['energies'] * vib_ref.INV_CM)
        e = vib_ref.HBAR * np.sqrt(vib_ref.ACC * np.abs(r['eigenvalues'])) * np.sign(r['eigenvalues'])
        assert np.array_equal(r['energies'], e) and r['zpe'] == 0.5 * e[e > 0].sum()
        assert np.all(np.diff(r['eigenvalues']) >= 0)
    assert np.array_equal(res[2]['hessian'], np.zeros((3, 3))) and res[2]['num_edges'] == 0   # the isolated atom


def test_undisplaced_results_are_compute_many_and_two_runs_are_identical(model, runs):
    systems, out = runs
    res, _ = out[2]
    args = _vib_args(systems)
    many = model.calc.compute_many(args[0], args[1], args[3], args[4])
    for r, one in zip(res, many):   # the batch-versus-single tolerances of test_batch_gpu
        assert set(r) == set(one) | {'atomic_energies', 'indices', 'hessian', 'asymmetry', 'eigenvalues', 'modes', 'energies', 'frequencies', 'zpe', 'status'}
        assert abs(r['energy'] - one['energy']) <= 1e-6 * abs(one['energy']) + 1e-6 and r['free_energy'] == r['energy']
        assert np.abs(r['forces'] - one['forces']).max() <= 2e-5 * max(1.0, np.abs(one['forces']).max())
        assert np.abs(r['atomic_energies'] - one['energies']).max() <= 1e-6 * max(1.0, np.abs(one['energies']).max())
        assert r['num_edges'] == one['num_edges']
        assert np.allclose(r['stress'], one['stress'], rtol=0, atol=1e-5 * max(1e-3, np.nanmax(np.abs(one['stress']), initial=0)),
                           equal_nan=True)
    again = model.calc.vibrations_many(*args, delta=DELTA, nfree=2, indices=[s[4] for s in systems])
    for x, y in zip(res, again):
        for key in ('hessian', 'eigenvalues', 'modes', 'energies', 'frequencies', 'forces'):
            assert np.array_equal(x[key], y[key]), key
        assert x['asymmetry'] == y['asymmetry'] and x['zpe'] == y['zpe'] and x['energy'] == y['energy']
    # the caller's arrays are as they were, and a small budget gives the same Hessians within the engine's force tolerance
    assert np.array_equal(args[1][0], model_systems()[0][1])
    small = model.calc.vibrations_many(*args, delta=DELTA, nfree=2, indices=[s[4] for s in systems], max_atoms_per_call=100)
    assert model.calc.vib_info['n_force_calls'] > 1
    for x, y in zip(res, small):
        # (each force of either run is within 2e-5 max(1, |F|) of the single-structure one: 4e-5 apart, two of them over 2 delta)
        assert np.abs(x['hessian'] - y['hessian']).max() <= 4e-5 * max(1.0, 2.0 * np.abs(x['forces']).max()) / DELTA


# ------------------------------------------------------------------------------------------------ surfaces
class _MassAtoms(_Atoms):
    def __init__(self, z, pos, cell, pbc, masses):
        super().__init__(z, pos, cell, pbc)
        self.masses = np.asarray(masses, float)

    def get_masses(self):
        return self.masses.copy()

    def set_positions(self, pos):
        raise AssertionError('vibrations_many_atoms writes nothing back')


def test_the_atoms_surface_and_validation(model, runs):
    systems, out = runs
    res, _ = out[2]
    numbers, positions, masses, cells, pbcs = _vib_args(systems)
    atoms = [_MassAtoms(z, p, c, pb, ms) for z, p, ms, c, pb in zip(numbers, positions, masses, cells, pbcs)]
    got = model.calc.vibrations_many_atoms(atoms, delta=DELTA, nfree=2, indices=[s[4] for s in systems])
    for x, y in zip(res, got):
        assert np.array_equal(x['hessian'], y['hessian']) and np.array_equal(x['eigenvalues'], y['eigenvalues'])
        assert np.array_equal(x['forces'], y['forces'])
    # a calculator that reports per-atom virials reports those of the undisplaced structures (an edge's share of the virial is
    # its force share times a distance below the 5 A cutoff: five times the batch-versus-single force tolerance)
    calc_v, _, _ = _calc(model.cfg, compute_atomic_virial=True)
    with_v = calc_v.vibrations_many(numbers, positions, masses, cells, pbcs, delta=DELTA, nfree=2, indices=[s[4] for s in systems])
    many_v = calc_v.compute_many(numbers, positions, cells, pbcs)
    for x, y, one in zip(res, with_v, many_v):
        assert np.abs(x['hessian'] - y['hessian']).max() <= 4e-5 * max(1.0, 2.0 * np.abs(x['forces']).max()) / DELTA   # (as for a small budget)
        assert y['stresses'].shape == one['stresses'].shape
        assert np.abs(y['stresses'] - one['stresses']).max() <= 1e-4 * max(1.0, np.abs(one['stresses']).max())
    with pytest.raises(ValueError, match='system 1: atom index 5 is out of range'):
        model.calc.vibrations_many(numbers, positions, masses, cells, pbcs, indices=[None, [5], None])
    with pytest.raises(ValueError, match='nfree'):
        model.calc.vibrations_many(numbers, positions, masses, cells, pbcs, nfree=3)
    with pytest.raises(ValueError, match='Model do not know atomic number: 79'):
        model.calc.vibrations_many([[79]], [np.zeros((1, 3))], [[197.0]], np.zeros((1, 3, 3)), [False] * 3)


def test_d3_sum_on_the_host_term_and_on_the_device_term(model, runs):
    """the device term's forces are the host term's bit for bit at fixed cells (test_d3_device_gpu) and the rows kernel adds them
    in a fixed order, so the Hessians are equal bit for bit.  The D3 share H(model + D3) - H(model) is the finite difference
    of the D3 forces alone but for fp64 rounding: the model's fp32 forces are the same bits in both runs (the same copies in
    the same slots), and each of the two matrices is within 8 x 2^-53 x sum_w |weight_w F_w| / delta of the exact combination of
    its forces (test_kernels_equal_the_restatement); the restatement's own D adds as much again: 32 x 2^-53 x max |F| / delta
    with F the summed forces."""
    from sevennet_amd.d3 import D3Calculator, SevenNetD3Calculator
    systems, out = runs
    plain, _ = out[2]
    calc = SevenNetD3Calculator((model.cfg, model.sd), file_type='model_instance', device=DEV, **D3_CUT)
    args = _vib_args(systems)
    kw = dict(delta=DELTA, nfree=2, indices=[s[4] for s in systems])
    host = calc.vibrations_many(*args, d3_term='host', **kw)
    info = dict(calc.vib_info)
    dev = calc.vibrations_many(*args, d3_term='device', **kw)
    assert calc.vib_info == info and info['n_force_calls'] == 1
    d3 = D3Calculator(**D3_CUT)
    for b, (h, d, p) in enumerate(zip(host, dev, plain)):
        assert np.isfinite(h['hessian']).all() and h['status'] == d['status'] == 'ok'
        assert np.array_equal(h['hessian'], d['hessian']) and np.array_equal(h['eigenvalues'], d['eigenvalues'])
        assert h['energy'] == d['energy'] and np.array_equal(h['forces'], d['forces'])
        z, pos, cell, pbc = args[0][b], args[1][b], args[3][b], args[4][b]
        alone = d3.compute(z, pos, cell, pbc)
        assert abs(h['energy'] - (p['energy'] + alone['energy'])) <= 1e-12 * abs(h['energy'])
        assert np.abs(h['forces'] - (p['forces'] + alone['forces'])).max() <= 1e-12 * max(1.0, np.abs(h['forces']).max())
        ref = vib_ref.vibrations(lambda q: d3.compute(z, q, cell, pbc)['forces'], pos, args[2][b], systems[b][4], DELTA, 2)
        share = h['hessian'] - p['hessian']
        fmax = np.abs(p['forces']).max() + np.abs(alone['forces']).max() + np.abs(h['hessian']).max() * 2 * DELTA   # (forces at the displaced copies)
        err, tol = np.abs(share - ref['hessian']).max(), 32 * EPS * fmax / DELTA
        print(f'system {b}: max |H(model + D3) - H(model) - H(D3)| {err:.3e} (bound {tol:.3e}), max |H(D3)| {np.abs(ref["hessian"]).max():.3e}')
        assert err <= tol
        if b < 2:
            assert np.abs(ref['hessian']).max() > 0 and not np.array_equal(h['hessian'], p['hessian'])   # the D3 share is in
