"""CPU: the fp64 restatement of the finite-difference rule (vib_ref) is exact on a quadratic potential and gives the spectrum of
a spring in closed form; the host side of sevennet_amd.vib (the plan of the copies, argument validation, the harmonic
prefactor, the ABI entries) does what it says without a device."""
import os
import re

import numpy as np
import pytest

import vib_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('snet_vib_displace', 'snet_vib_rows', 'snet_vib_finish')


def test_abi_entries():
    from sevennet_amd import _lib
    from sevennet_amd.build import STATIC_SOURCES
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'snet_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        args = re.search(r'\bint %s\s*\((.*?)\)\s*;' % name, text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(args.split(',')), name
        assert hasattr(lib, name), name
    assert 'snet_vib.hip' in STATIC_SOURCES
    assert _lib.ABI_VERSION == 4


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('nfree', [2, 4])
def test_central_differences_are_exact_on_a_quadratic_potential(nfree):
    """E = x^T K x / 2: F is linear in x, so both stencils give K but for rounding.  A force is known to 2^-53 |F| relative (its
    own rounding: the row of K times x is summed in fp64, an error of a few 2^-53 max|F|), the stencil combines at most four
    of them with weights that sum to at most 1.5 / delta, and displacing x rounds x + q delta: 16 x 2^-53 max|F| / delta
    covers them."""
    rng = np.random.default_rng(3)
    n, delta = 6, 0.01
    K = vib_ref.random_spd_like(rng, 3 * n)
    x0 = rng.normal(0.0, 1.0, (n, 3))
    pos = x0 + rng.normal(0.0, 0.3, (n, 3))
    force = vib_ref.quadratic(K, x0)
    fmax = max(np.abs(force(vib_ref.displaced(pos, a, i, q, delta))).max() for a in range(n) for i in range(3) for q in (-2, 2))
    res = vib_ref.vibrations(force, pos, np.ones(n), None, delta, nfree)
    err, tol = np.abs(res['hessian'] - K).max(), 16 * 2.0 ** -53 * fmax / delta
    print(f'nfree {nfree}: max |H - K| = {err:.3e} (bound {tol:.3e}), asymmetry {res["asymmetry"]:.3e}')
    assert err <= tol
    assert np.array_equal(res['hessian'], res['hessian'].T) and np.array_equal(res['hessian_mw'], res['hessian_mw'].T)
    assert res['asymmetry'] <= 2 * tol
    # a subset: the block of K of those atoms
    idx = np.array([4, 1])
    sub = vib_ref.vibrations(force, pos, np.ones(n), idx, delta, nfree)
    rows = (3 * idx[:, None] + np.arange(3)).reshape(-1)
    assert np.abs(sub['hessian'] - K[np.ix_(rows, rows)]).max() <= tol


def test_a_spring_has_its_closed_form_spectrum_and_a_negative_curvature_comes_out_negative():
    """two atoms on a spring of constant k along x: one mode with lambda = k / mu, mu the reduced mass, five zero modes;
    h nu = hbar sqrt(ACC k / mu).  With k < 0 the same mode is reported negative and is not in the zero-point energy."""
    m1, m2, k = 12.011, 1.008, 31.7
    mu = m1 * m2 / (m1 + m2)
    for sign in (1.0, -1.0):
        K = np.zeros((6, 6))
        K[0, 0] = K[3, 3] = sign * k
        K[0, 3] = K[3, 0] = -sign * k
        # plus a weak positive curvature of y of atom 1 alone, so that zpe has something to keep when sign < 0
        K[4, 4] = 2.0
        res = vib_ref.vibrations(vib_ref.quadratic(K), np.array([[0.0, 0, 0], [1.1, 0, 0]]), [m1, m2], None, 0.01, 2)
        want = vib_ref.HBAR * np.sqrt(vib_ref.ACC * k / mu)
        side = vib_ref.HBAR * np.sqrt(vib_ref.ACC * 2.0 / m2)
        e = res['energies']
        stretch = e[-1] if sign > 0 else e[0]
        assert abs(stretch - sign * want) <= 1e-12 * want, (stretch, want)
        assert abs(res['frequencies'][-1 if sign > 0 else 0] - sign * want * vib_ref.INV_CM) <= 1e-12 * want * vib_ref.INV_CM
        positive = e[e > 1e-6]   # (a zero mode: |lambda| of the order 1e-15 from rounding, h nu of the order 1e-9 eV)
        assert len(positive) == (2 if sign > 0 else 1)
        zpe_want = 0.5 * (side + (want if sign > 0 else 0.0))
        tiny = 0.5 * np.abs(e[np.abs(e) <= 1e-6]).sum()   # the zero modes: whatever sign rounding gave them
        assert abs(res['zpe'] - zpe_want) <= 1e-12 * zpe_want + tiny
        if sign < 0:
            assert e[0] < 0 and res['eigenvalues'][0] < 0
            assert res['zpe'] < 0.5 * want   # the negative direction is not counted
        # modes: orthonormal, row k belongs to eigenvalue k
        M = res['modes'].reshape(6, 6)
        assert np.abs(M @ M.T - np.eye(6)).max() <= 1e-12
        assert np.abs(res['hessian_mw'] @ M[-1] - res['eigenvalues'][-1] * M[-1]).max() <= 1e-10


def test_the_driver_spectrum_is_the_restatements():
    from sevennet_amd import vib
    assert (vib.HBAR, vib.INV_CM, vib.ACC) == (vib_ref.HBAR, vib_ref.INV_CM, vib_ref.ACC) and vib.STENCIL == vib_ref.STENCIL
    rng = np.random.default_rng(5)
    Hm = vib_ref.random_spd_like(rng, 9)
    got, want = vib.spectrum(Hm), vib_ref.spectrum(Hm)
    for key in ('eigenvalues', 'modes', 'energies', 'frequencies'):
        assert np.array_equal(got[key], want[key]), key
    assert got['zpe'] == want['zpe'] and (got['energies'] < 0).any() and got['modes'].shape == (9, 3, 3)
    bad = vib.spectrum(np.full((6, 6), np.nan))
    assert np.isnan(bad['eigenvalues']).all() and np.isnan(bad['zpe']) and bad['modes'].shape == (6, 2, 3)


# ------------------------------------------------------------------------------------------------ the plan
PLAN_N = [1, 5, 64, 300]
PLAN_SEL = [np.arange(1), np.arange(5), np.array([3, 60, 7, 21, 0, 63, 40]), np.arange(300)]


@pytest.mark.parametrize('nfree', [2, 4])
@pytest.mark.parametrize('budget', [1, 40, 1000, 10 ** 6])
def test_plan_copies(nfree, budget):
    from sevennet_amd.vib import STENCIL, plan_copies
    plan = plan_copies(PLAN_N, PLAN_SEL, nfree, budget)
    n = np.array(PLAN_N)
    seen = {}
    assert len(plan.slot_system) == sum(np.sum(plan.slot_system == b) for b in range(4))
    for call in plan.calls:
        assert len(call.ids) == len(call.desc) and len(set(call.ids.tolist())) == len(call.ids)
        assert np.array_equal(plan.slot_system[call.ids], call.desc[:, 0])       # a copy sits in a slot of its own system
        assert np.array_equal(call.ids, np.sort(call.ids))
        in_group = np.zeros(len(call.desc), bool)
        for j0, b, r in call.groups:   # whole, adjacent, in the stated order of q
            a = PLAN_SEL[b][r // 3]
            assert call.desc[j0:j0 + nfree].tolist() == [[b, a, r % 3, q] for q in STENCIL[nfree]]
            assert not in_group[j0:j0 + nfree].any()
            in_group[j0:j0 + nfree] = True
        rest = np.nonzero(~in_group)[0]
        assert [(int(j), int(call.desc[j, 0])) for j in rest] == [(int(j), int(b)) for j, b in call.base]
        assert (call.desc[rest, 3] == 0).all() and (call.desc[in_group, 3] != 0).all()
        atoms = int(n[call.desc[:, 0]].sum())
        assert atoms == call.n_atoms
        assert atoms <= budget or len(call.groups) + len(call.base) == 1, (atoms, budget)
        for d in call.desc.tolist():
            key = tuple(d) if d[3] != 0 else (d[0], -1, -1, 0)
            seen[key] = seen.get(key, 0) + 1
    want = {(b, -1, -1, 0) for b in range(4)} | {(b, int(a), i, q) for b in range(4) for a in PLAN_SEL[b] for i in range(3)
                                                  for q in STENCIL[nfree]}
    assert set(seen) == want and set(seen.values()) == {1}
    assert sum(len(c.ids) for c in plan.calls) == sum(nfree * 3 * len(s) + 1 for s in PLAN_SEL)
    if budget == 10 ** 6 and nfree == 2:
        assert len(plan.calls) == 1
    # the calls before the layout thins out all use the same slots
    if budget == 10 ** 6 and nfree == 4:
        assert len(plan.calls) == 2 and len(plan.calls[0].ids) >= len(plan.calls[1].ids)


def test_plan_slots_are_proportional_to_the_work():
    """24 equal systems in a budget that takes a seventh of their copies: every call but the last uses the same slots"""
    from sevennet_amd.vib import plan_copies
    sel = [np.arange(63)] * 24
    plan = plan_copies([63] * 24, sel, 2, 32768)
    layouts = {c.ids.tobytes() for c in plan.calls[:-1]}
    assert len(layouts) == 1 and max(c.n_atoms for c in plan.calls) <= 32768
    # 24 x 63 x (2 g + 1) <= 32768 allows g = 10 row groups per system and call: ceil(189 / 10) = 19 calls
    assert len(plan.calls) == 19 and [len(c.groups) for c in plan.calls] == [240] * 18 + [24 * 9]
    assert [len(c.base) for c in plan.calls] == [0] * 18 + [24]


# ------------------------------------------------------------------------------------------------ validation
def test_validation_names_the_system():
    from sevennet_amd.vib import validate_vib_inputs
    n = [2, 3]
    masses = [np.ones(2), np.ones(3)]
    ok = dict(n_atoms=n, masses=masses, indices=None, delta=0.01, nfree=2, max_atoms_per_call=100)

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            validate_vib_inputs(**dict(ok, **kw))

    m, sel = validate_vib_inputs(**ok)
    assert [s.tolist() for s in sel] == [[0, 1], [0, 1, 2]]
    m, sel = validate_vib_inputs(**dict(ok, masses=np.arange(1.0, 6.0), indices=[[1], np.array([True, False, True])]))
    assert [s.tolist() for s in sel] == [[1], [0, 2]] and m[1].tolist() == [3.0, 4.0, 5.0]
    for d in (0.0, -0.01, float('nan'), float('inf'), None):
        bad('delta', delta=d)
    for f in (1, 3, 6, True, 2.5):
        bad('nfree', nfree=f)
    for c in (0, -3, 2.5, None, True):
        bad('max_atoms_per_call', max_atoms_per_call=c)
    bad('system 1: masses must be finite and positive', masses=[np.ones(2), np.array([1.0, 0.0, 1.0])])
    bad('system 0: masses must be finite and positive', masses=[np.array([np.nan, 1.0]), np.ones(3)])
    bad('system 1: 2 masses but 3 atoms', masses=[np.ones(2), np.ones(2)])
    bad('system 1: an index mask of shape', indices=[None, np.array([True, False])])
    bad('system 0: atom index 2 is out of range', indices=[[0, 2], None])
    bad('system 1: atom index -1 is out of range', indices=[None, [-1]])
    bad('system 1: an atom index is given more than once', indices=[None, [2, 0, 2]])
    bad('system 0: no atom is selected', indices=[[], None])
    bad('system 1: no atom is selected', indices=[None, np.zeros(3, bool)])
    bad('system 0: the displaced atoms are given as', indices=[[0.5], None])
    bad('one entry per system', indices=[None])


# ------------------------------------------------------------------------------------------------ the prefactor
def test_harmonic_prefactor_in_closed_form():
    from sevennet_amd.vib import HBAR, harmonic_prefactor
    h = 2.0 * np.pi * HBAR * 1e-3   # eV per THz
    lo = np.array([3.0, 5.0, 7.0]) * h          # 3, 5 and 7 THz at the minimum
    hi = np.array([-2.0, 4.0, 6.0]) * h         # one imaginary mode and 4, 6 THz at the saddle
    assert abs(harmonic_prefactor(lo, hi) - 105.0 / 24.0) <= 1e-12 * 105.0 / 24.0
    assert abs(harmonic_prefactor(np.concatenate([[-1e-9, 0.0], lo]), hi) - 105.0 / 24.0) <= 1e-12 * 105.0 / 24.0   # non-positive modes are skipped
    assert abs(harmonic_prefactor([0.01], [-0.02]) - 0.01 / h) <= 1e-12 * 0.01 / h
    with pytest.raises(ValueError, match='3 positive modes at the minimum and 3 at the saddle'):
        harmonic_prefactor(lo, np.abs(hi))
    with pytest.raises(ValueError, match='exactly one more'):
        harmonic_prefactor(lo[:2], hi)
    with pytest.raises(ValueError, match='finite'):
        harmonic_prefactor([np.nan, 1.0], [1.0])
