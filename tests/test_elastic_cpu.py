"""CPU: the fp64 restatement of the elastic rule (elastic_ref) on a smooth pair potential -- the relaxed-ion formula against
brute-force relaxation of the strained cells -- and the host side of sevennet_amd.elastic (the plan of the copies, the strained
cells, the pseudo-inverse, the polycrystal averages, argument validation, the ABI entries) without a device."""
import hashlib
import os
import re

import numpy as np
import pytest

import elastic_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('snet_el_strain', 'snet_el_rows', 'snet_el_finish')


def test_abi_entries():
    from sevennet_amd import _lib
    from sevennet_amd.build import STATIC_SOURCES
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'snet_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        args = re.search(r'\bint %s\s*\((.*?)\)\s*;' % name, text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(args.split(',')), name
        assert hasattr(lib, name), name
    assert 'snet_elastic.hip' in STATIC_SOURCES
    assert _lib.ABI_VERSION == 4   # symbols are only added


# ------------------------------------------------------------------------------------------------ the restatement
def _triclinic():
    """three atoms in a triclinic cell, rattled: no symmetry, so the internal-strain tensor is full"""
    cell = np.array([[4.1, 0.0, 0.0], [0.7, 3.8, 0.0], [0.4, -0.5, 4.4]])
    frac = np.array([[0.03, 0.05, 0.02], [0.41, 0.35, 0.38], [0.71, 0.68, 0.77]])
    return frac @ cell, cell


def test_pair_potential_forces_and_virial_are_the_energy_derivatives():
    """the analytic forces and virial of the test potential against central differences of its energy: a step of 1e-5 leaves a
    truncation of the order 1e-10 relative and a rounding of 2^-53 |E| / 1e-5, some 1e-11 here"""
    pot = elastic_ref.PairPotential()
    pos, cell = _triclinic()
    e0, f, w = pot.eval(pos, cell)
    h = 1e-5
    for a in range(3):
        for k in range(3):
            p, m = pos.copy(), pos.copy()
            p[a, k] += h
            m[a, k] -= h
            assert abs(-(pot.eval(p, cell)[0] - pot.eval(m, cell)[0]) / (2 * h) - f[a, k]) <= 1e-8
    sigma = elastic_ref.stress_of(w, None, abs(np.linalg.det(cell)))
    for j in range(6):   # sigma_j = (1 / V) dE / d epsilon_j (engineering shear)
        ep = pot.eval(elastic_ref.strained(pos, j, 1, h), elastic_ref.strained(cell, j, 1, h))[0]
        em = pot.eval(elastic_ref.strained(pos, j, -1, h), elastic_ref.strained(cell, j, -1, h))[0]
        assert abs((ep - em) / (2 * h) / abs(np.linalg.det(cell)) - sigma[j]) <= 1e-8
    assert np.abs(sigma).max() > 1e-3   # a residual stress: S is legitimately asymmetric here


def test_strained_rows_are_x_times_F():
    rng = np.random.default_rng(1)
    x = rng.normal(0.0, 2.0, (7, 3))
    for j in range(6):
        for q in (-2, -1, 1, 2):
            F = np.eye(3) + (q * 0.01) * elastic_ref.pattern(j)
            assert np.abs(elastic_ref.strained(x, j, q, 0.01) - x @ F).max() <= 4 * 2.0 ** -53 * np.abs(x).max()
            assert np.array_equal(F, F.T)
        assert np.array_equal(elastic_ref.strained(x, j, 0, 0.01), x)
    assert np.array_equal(elastic_ref.pattern(3), np.array([[0, 0, 0], [0, 0, 0.5], [0, 0.5, 0]]))   # yz: gamma = delta


def test_relaxed_ion_formula_equals_brute_force_relaxation():
    """S_rel = S - L Phi+ L^T / V against central differences of the stresses of strained cells whose ions were relaxed.

    Both are differences of step delta = 1e-4 (and the Hessian one of step ion_delta), so each carries a truncation error c h^2;
    halving the steps changes a result by (3/4) c h^2, so twice that change bounds the error of each.  The relaxed copies stop at
    a residual force f: their stress is off by |L Phi+| f / V at most to first order, and the difference by that over delta.  The
    bound is the sum of the three, nothing is taken from the difference under test."""
    pot = elastic_ref.PairPotential()
    pos, cell = _triclinic()
    pos, f0 = elastic_ref.relax_ions(pot, pos, cell)
    assert f0 < 3e-10
    V = abs(np.linalg.det(cell))
    delta, ion_delta = 1e-4, 0.01
    fn = pot.eval_fn()
    a = elastic_ref.elastic(fn, pos, cell, delta, 2, relax_ions=True, ion_delta=ion_delta)
    a2 = elastic_ref.elastic(fn, pos, cell, delta / 2, 2, relax_ions=True, ion_delta=ion_delta / 2)
    bf, res = elastic_ref.brute_force_relaxed(pot, pos, cell, delta)
    bf2, res2 = elastic_ref.brute_force_relaxed(pot, pos, cell, delta / 2)
    gain = np.abs(a['L'] @ elastic_ref.pseudo_inverse(a['hessian'])).max()
    t_formula, t_brute = 2 * np.abs(a['stress_strain'] - a2['stress_strain']).max(), 2 * np.abs(bf - bf2).max()
    t_resid = gain * max(res, res2) / (V * delta / 2)
    err = np.abs(a['stress_strain'] - bf).max()
    corr = np.abs(a['stress_strain'] - a['stress_strain_clamped']).max()
    sigma0 = np.abs(fn(pos, cell)[1]).max()
    print(f'max |S_rel - brute force| = {err:.3e} eV/A^3 (bound {t_formula + t_brute + t_resid:.3e} = {t_formula:.3e} formula + '
          f'{t_brute:.3e} brute force + {t_resid:.3e} residual forces {max(res, res2):.1e}); correction {corr:.3e}, |sigma_0| {sigma0:.3e}')
    assert err <= t_formula + t_brute + t_resid
    assert corr > 100 * (t_formula + t_brute + t_resid)   # the correction is far above what the comparison resolves
    # the relaxed tensor is the symmetric part, and the correction itself is symmetric: the asymmetry is that of the clamped S
    assert np.array_equal(a['elastic_tensor'], a['elastic_tensor'].T)
    assert abs(a['asymmetry'] - elastic_ref.finish(a['stress_strain_clamped'])[1]) <= 1e-9


# ------------------------------------------------------------------------------------------------ host side of the driver
def test_strain_rows_and_plan_cells_have_the_restatements_bits():
    from sevennet_amd.elastic import plan_elastic, strain_rows
    rng = np.random.default_rng(2)
    x = rng.normal(0.0, 3.0, (5, 3))
    for j in range(6):
        for q in (-2, -1, 0, 1, 2):
            assert np.array_equal(strain_rows(x, j, q, 0.005), elastic_ref.strained(x, j, q, 0.005))
    cells = rng.normal(0.0, 1.0, (2, 3, 3)) + 4.0 * np.eye(3)
    plan = plan_elastic([3, 1], cells, 0.005, 4, 10 ** 6)
    for s, (b, j, q) in enumerate(plan.slot_desc.tolist()):
        assert plan.slot_system[s] == b
        assert np.array_equal(plan.slot_cells[s], elastic_ref.strained(cells[b], j, q, 0.005))
        assert plan.slot_volumes[s] == abs(np.linalg.det(plan.slot_cells[s]))


@pytest.mark.parametrize('nfree', [2, 4])
@pytest.mark.parametrize('budget', [1, 40, 1000, 10 ** 6])
def test_plan_is_complete(nfree, budget):
    """every (system, j, q) and every unstrained copy is planned exactly once, in a slot of its own whose descriptor it matches;
    groups are whole, adjacent and in the stencil's order; a call stays within the budget unless it holds a single item"""
    from sevennet_amd.elastic import plan_elastic
    from sevennet_amd.vib import STENCIL
    n = np.array([1, 5, 64, 300])
    cells = np.tile(5.0 * np.eye(3), (4, 1, 1))
    plan = plan_elastic(n, cells, 0.005, nfree, budget)
    per = 6 * nfree + 1
    assert len(plan.slot_system) == 4 * per and np.array_equal(plan.slot_system, np.repeat(np.arange(4), per))
    seen = {}
    for call in plan.calls:
        assert call.desc.shape == (len(call.ids), 3) and len(set(call.ids.tolist())) == len(call.ids)
        assert np.array_equal(plan.slot_desc[call.ids], call.desc)     # a copy sits in the slot with its own strained cell
        in_group = np.zeros(len(call.desc), bool)
        for j0, b, j in call.groups:
            assert call.desc[j0:j0 + nfree].tolist() == [[b, j, q] for q in STENCIL[nfree]]
            assert not in_group[j0:j0 + nfree].any()
            in_group[j0:j0 + nfree] = True
        rest = np.nonzero(~in_group)[0]
        assert [(int(c), int(call.desc[c, 0])) for c in rest] == [(int(c), int(b)) for c, b in call.base]
        assert (call.desc[rest, 2] == 0).all() and (call.desc[in_group, 2] != 0).all()
        atoms = int(n[call.desc[:, 0]].sum())
        assert atoms == call.n_atoms and (atoms <= budget or len(call.groups) + len(call.base) == 1)
        for b, j, q in call.desc.tolist():
            key = (b, j, q) if q != 0 else (b, -1, 0)
            seen[key] = seen.get(key, 0) + 1
    want = {(b, -1, 0) for b in range(4)} | {(b, j, q) for b in range(4) for j in range(6) for q in STENCIL[nfree]}
    assert set(seen) == want and set(seen.values()) == {1}
    assert sum(len(c.ids) for c in plan.calls) == 4 * per
    if budget == 10 ** 6:
        assert len(plan.calls) == 1


def _digest(plan):
    h = hashlib.sha256()
    h.update(plan.slot_system.astype(np.int64).tobytes() + plan.n_groups.astype(np.int64).tobytes())
    for c in plan.calls:
        for a in (c.ids.astype(np.int64), c.desc.astype(np.int32), c.groups.astype(np.int32), np.asarray(c.base, np.int64).reshape(-1)):
            h.update(a.tobytes() + b'|')
        h.update(str(c.n_atoms).encode())
    return h.hexdigest()[:16]


# digests of plan_copies' output taken before it learned `n_groups` (the inputs of test_vib_cpu.test_plan_copies)
VIB_PLAN_DIGESTS = {(2, 1): 'e9ac2e877ac98425', (2, 40): 'd5c5ce543a32bef7', (2, 1000): '271256a7b0bded5b', (2, 1000000): 'a01e0ec124ca731c',
                    (4, 1): '09bd0a253e5172f9', (4, 40): 'd71a7bef5ee6db65', (4, 1000): 'b73e654e763b3e5a', (4, 1000000): '59524b9250ac8f92'}


def test_plan_copies_for_vibrations_is_unchanged():
    from sevennet_amd.vib import plan_copies
    n = [1, 5, 64, 300]
    sel = [np.arange(1), np.arange(5), np.array([3, 60, 7, 21, 0, 63, 40]), np.arange(300)]
    got = {(nfree, budget): _digest(plan_copies(n, sel, nfree, budget)) for nfree in (2, 4) for budget in (1, 40, 1000, 10 ** 6)}
    assert got == VIB_PLAN_DIGESTS


def test_pseudo_inverse_annihilates_translations():
    from sevennet_amd.elastic import ion_pseudo_inverse, translations
    rng = np.random.default_rng(4)
    n = 5
    A = rng.normal(0.0, 1.0, (3 * n, 3 * n))
    T = translations(n)
    P = np.eye(3 * n) - T @ T.T
    phi = P @ (A @ A.T + 0.5 * np.eye(3 * n)) @ P        # translation-invariant, positive on the complement
    plus, lam = ion_pseudo_inverse(phi)
    assert np.abs(T.T @ T - np.eye(3)).max() <= 1e-15
    assert np.abs(plus @ T).max() <= 1e-12 * np.abs(plus).max() and np.abs(T.T @ plus).max() <= 1e-12 * np.abs(plus).max()
    assert np.abs(plus @ phi - P).max() <= 1e-10 and np.abs(plus - plus.T).max() <= 1e-12 * np.abs(plus).max()
    assert len(lam) == 3 * n - 3 and lam[0] >= 0.5 - 1e-9
    assert np.abs(plus - elastic_ref.pseudo_inverse(phi)).max() <= 1e-10 * np.abs(plus).max()
    # a rigid shift added to the forces' response changes nothing: L Phi+ L^T sees only the complement
    L = rng.normal(0.0, 1.0, (6, 3 * n))
    shift = rng.normal(0.0, 1.0, (6, 3)) @ T.T
    assert np.abs((L + shift) @ plus @ (L + shift).T - L @ plus @ L.T).max() <= 1e-10
    # a soft direction at or below the floor: refused; one atom: nothing to relax
    soft = phi - (lam[0] - 1e-9) * P
    assert ion_pseudo_inverse(soft, floor=1e-6)[0] is None and ion_pseudo_inverse(soft, floor=0.0)[0] is not None
    assert ion_pseudo_inverse(-phi)[0] is None
    one, lam1 = ion_pseudo_inverse(np.zeros((3, 3)))
    assert np.array_equal(one, np.zeros((3, 3))) and len(lam1) == 0


def test_moduli_closed_forms():
    from sevennet_amd.elastic import GPA, moduli
    assert GPA == 160.21766208 == elastic_ref.GPA
    c11, c12, c44 = 1.05, 0.40, 0.50
    C = np.zeros((6, 6))
    C[:3, :3] = c12
    C[np.arange(3), np.arange(3)] = c11
    C[np.arange(3, 6), np.arange(3, 6)] = c44
    m = moduli(C)
    K, gv, gr = (c11 + 2 * c12) / 3, (c11 - c12 + 3 * c44) / 5, 5 * (c11 - c12) * c44 / (4 * c44 + 3 * (c11 - c12))
    for key in ('voigt', 'reuss', 'hill'):
        assert abs(m['bulk_modulus'][key] - K) <= 1e-14
    assert abs(m['shear_modulus']['voigt'] - gv) <= 1e-14 and abs(m['shear_modulus']['reuss'] - gr) <= 1e-14
    assert abs(m['shear_modulus']['hill'] - 0.5 * (gv + gr)) <= 1e-14 and gr < gv
    g = 0.5 * (gv + gr)
    assert abs(m['youngs_modulus'] - 9 * K * g / (3 * K + g)) <= 1e-14 and abs(m['poisson_ratio'] - (3 * K - 2 * g) / (2 * (3 * K + g))) <= 1e-14
    assert m['stable'] and np.abs(m['compliance'] @ C - np.eye(6)).max() <= 1e-14
    ref = elastic_ref.moduli(C)
    assert np.allclose(list(m['bulk_modulus'].values()), ref['bulk'], rtol=0, atol=1e-14)
    assert np.allclose(list(m['shear_modulus'].values()), ref['shear'], rtol=0, atol=1e-14)
    # isotropic: c44 = (c11 - c12) / 2 gives Voigt = Reuss
    C[np.arange(3, 6), np.arange(3, 6)] = 0.5 * (c11 - c12)
    iso = moduli(C)
    assert abs(iso['shear_modulus']['voigt'] - iso['shear_modulus']['reuss']) <= 1e-14
    assert abs(iso['shear_modulus']['hill'] - 0.5 * (c11 - c12)) <= 1e-14 and abs(iso['bulk_modulus']['voigt'] - iso['bulk_modulus']['reuss']) <= 1e-14
    # c12 > c11: not stable; a NaN tensor: NaN throughout
    C[:3, :3] = 2.0
    C[np.arange(3), np.arange(3)] = c11
    assert not moduli(C)['stable']
    bad = moduli(np.full((6, 6), np.nan))
    assert np.isnan(bad['bulk_modulus']['hill']) and np.isnan(bad['compliance']).all() and not bad['stable']


def test_validation_names_the_system():
    from sevennet_amd.elastic import validate_elastic_inputs
    cells = np.tile(4.0 * np.eye(3), (2, 1, 1))
    ok = dict(n_atoms=[2, 3], cells=cells, pbcs=np.ones((2, 3), bool), delta=0.005, nfree=2, max_atoms_per_call=100)

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            validate_elastic_inputs(**dict(ok, **kw))

    validate_elastic_inputs(**ok)
    for d in (0.0, -0.01, float('nan'), float('inf'), None, True):
        bad('delta', delta=d)
    bad('ion_delta', ion_delta=0.0)
    for f in (1, 3, 6, True, 2.5):
        bad('nfree', nfree=f)
    for c in (0, -3, 2.5, None, True):
        bad('max_atoms_per_call', max_atoms_per_call=c)
    bad('system 1: an elastic tensor needs a fully periodic system', pbcs=np.array([[1, 1, 1], [1, 1, 0]], bool))   # a slab
    bad('system 0: an elastic tensor needs a fully periodic system', pbcs=np.zeros((2, 3), bool))                   # a molecule
    flat = cells.copy()
    flat[1, 2] = flat[1, 1]
    bad('system 1: the cell is singular', cells=flat)
    flat[0, 0, 0] = np.nan
    bad('system 0: the cell is singular or not finite', cells=flat)
