"""CPU: the fp64 restatement of the phonon rule (phonon_ref) meets the closed form of a diatomic chain, also where an atom sits
exactly half a supercell away, and the commensurate-q identity; the 27-candidate image rule equals a brute-force search on reduced
cells; the host side of sevennet_amd.phonon (validation, the reduced-cell check, thermodynamics, the density of states, the band
path, the ABI entries) does what it says without a device."""
import os
import re

import numpy as np
import pytest

import phonon_ref
import vib_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('snet_ph_rows', 'snet_ph_finish', 'snet_ph_images', 'snet_ph_dynmat')


def test_abi_entries():
    from sevennet_amd import _lib
    from sevennet_amd.build import STATIC_SOURCES
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'snet_hip.h')).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        args = re.search(r'\bint %s\s*\((.*?)\)\s*;' % name, text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(args.split(',')), name
        assert hasattr(lib, name), name
    assert 'snet_phonon.hip' in STATIC_SOURCES


# ------------------------------------------------------------------------------------------------ the chain
def _chain_D(n, q_frac, acoustic=True):
    """D(q) of the chain from the restatement, with Phi = the home rows of the supercell's spring matrix"""
    pos, cell, masses = phonon_ref.chain_cell()
    pos_sc, S = phonon_ref.supercell(pos, cell, (n, 1, 1))
    _, Phi = phonon_ref.sum_rule(phonon_ref.chain_hessian(n)[:6], 2, acoustic)
    images, _ = phonon_ref.images_brute(pos_sc, S, 2)
    q = phonon_ref.q_cartesian([q_frac, 0.0, 0.0], cell)
    return phonon_ref.dynmat(Phi, pos_sc, S, 2, masses, images, q), images


@pytest.mark.parametrize('n', [2, 3, 4])
def test_restatement_meets_the_closed_form_of_the_diatomic_chain(n):
    """within 1e-12 of the largest eigenvalue; at n = 2 the second neighbour is exactly half a supercell away: two images, half the
    weight each"""
    for q in (0.0, 0.13, 0.37, 0.5):
        (R, D, herm, _, _), images = _chain_D(n, q)
        lam = np.linalg.eigvalsh(D)
        want = np.sort(np.concatenate([np.zeros(4), phonon_ref.chain_closed_form(q)]))
        err = np.abs(lam - want).max()
        print(f'n {n}, q {q}: max |d lambda| {err:.3e} of {want.max():.3e}, hermiticity {herm:.3e}')
        assert err <= 1e-12 * want.max()
        assert herm <= 1e-12 * want.max() and np.array_equal(D, D.conj().T)
    if n == 2:
        assert images[(0, 2)] == [(-1, 0, 0), (0, 0, 0)] and images[(1, 3)] == [(-1, 0, 0), (0, 0, 0)]   # the tie
        assert images[(0, 1)] == [(0, 0, 0)] and images[(0, 3)] == [(-1, 0, 0)]
    elif n == 3:
        assert images[(0, 3)] == [(-1, 0, 0), (0, 0, 0)] and images[(0, 2)] == [(0, 0, 0)] and images[(0, 4)] == [(-1, 0, 0)]   # (1.5 a is half of 3 a)
    else:
        assert images[(0, 4)] == [(-1, 0, 0), (0, 0, 0)] and images[(0, 2)] == [(0, 0, 0)]   # (n = 4: the cell two away is the tie)


@pytest.mark.parametrize('n', [2, 3, 4])
def test_commensurate_spectra_are_the_supercell_gamma_spectrum(n):
    """the union of the spectra of D(q) at q = k / n, k = 0 .. n - 1, equals the spectrum of the mass-weighted supercell Hessian"""
    _, _, masses = phonon_ref.chain_cell()
    K = phonon_ref.chain_hessian(n)
    w = np.repeat(1.0 / np.sqrt(np.tile(masses, n)), 3)
    want = np.linalg.eigvalsh(K * (w[:, None] * w[None, :]))
    got = np.sort(np.concatenate([np.linalg.eigvalsh(_chain_D(n, k / n, acoustic=False)[0][1]) for k in range(n)]))
    print(f'n {n}: max |d lambda| {np.abs(got - want).max():.3e} of {want.max():.3e}')
    assert np.abs(got - want).max() <= 1e-12 * want.max()


def test_sum_rule_and_rows_of_the_restatement():
    rng = np.random.default_rng(2)
    m, N = 2, 6
    Phi = rng.normal(0.0, 1.0, (3 * m, 3 * N))
    asr, fixed = phonon_ref.sum_rule(Phi, m, True)
    P4 = Phi.reshape(m, 3, N, 3)
    assert abs(asr - np.abs(P4.sum(2)).max()) <= 1e-14 * np.abs(Phi).sum()
    assert np.abs(fixed.reshape(m, 3, N, 3).sum(2)).max() <= 1e-14 * np.abs(Phi).sum()
    for a in range(m):
        others = [j for j in range(N) if j != a]
        assert np.array_equal(fixed.reshape(m, 3, N, 3)[a][:, others], P4[a][:, others])
    assert phonon_ref.sum_rule(Phi, m, False)[1].tobytes() == Phi.tobytes()
    # rows: a quadratic potential over the supercell gives its home rows back, within the bound of test_vib_cpu, 16 x 2^-53 x
    # max |F| / delta (no force is larger than 12 delta times the largest sum_w |weight_w F_w| / delta: the weights are >= 1 / 12)
    pos = rng.normal(0.0, 1.0, (N, 3))
    K = vib_ref.random_spd_like(rng, 3 * N)
    for nfree in (2, 4):
        got, scale = phonon_ref.force_constants(vib_ref.quadratic(K, pos), pos + rng.normal(0.0, 0.1, (N, 3)), m, 0.01, nfree, with_scale=True)
        assert got.shape == (3 * m, 3 * N) and np.abs(got - K[:3 * m]).max() <= 16 * 2.0 ** -53 * 12 * scale.max()


# ------------------------------------------------------------------------------------------------ cells and images
A = 3.9
CUBIC = np.eye(3) * A
FCC = np.array([[0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]]) * A
HEX = np.array([[1.0, 0.0, 0.0], [-0.5, np.sqrt(3.0) / 2.0, 0.0], [0.0, 0.0, 1.6]]) * A
LATTICES = {'cubic': CUBIC, 'fcc': FCC, 'hex': HEX}


def test_reduced_cell_check():
    from sevennet_amd.phonon import is_reduced
    for name, C in LATTICES.items():
        for reps in ((1, 1, 1), (2, 2, 2), (3, 3, 3)):
            assert is_reduced(np.array(reps)[:, None] * C), (name, reps)
        sheared = C.copy()
        sheared[2] = sheared[2] + 2.0 * sheared[0]
        assert not is_reduced(sheared), name
    assert not is_reduced(np.array([4, 1, 1])[:, None] * HEX)   # (4 a1 + a2 is shorter than 4 a1: unequal repeats of a skew cell)
    assert is_reduced(np.diag([9.0, 1.0, 1.0]))                 # (orthogonal rows are reduced whatever their lengths)


IMAGE_CASES = [('cubic', (1, 1, 1)), ('cubic', (2, 2, 2)), ('cubic', (3, 2, 1)), ('fcc', (1, 1, 1)), ('fcc', (2, 2, 2)), ('fcc', (3, 3, 3)),
               ('hex', (1, 1, 1)), ('hex', (2, 2, 2)), ('hex', (3, 3, 2))]


@pytest.mark.parametrize('name,reps', IMAGE_CASES)
def test_the_27_candidates_hold_the_brute_force_sets(name, reps):
    """two atoms per cell, rattled: the kept translations of the wrapped 27-candidate rule equal those of a search over {-3..3}^3 of
    the unwrapped pair; and on the perfect lattice, where equally near images are ties"""
    from sevennet_amd.phonon import is_reduced
    C = LATTICES[name]
    S = np.array(reps)[:, None] * C
    assert is_reduced(S)
    rng = np.random.default_rng(7)
    basis = np.array([[0.0, 0.0, 0.0], [0.25, 0.25, 0.25]]) @ C
    for rattle in (0.0, 0.05):
        pos_sc, S2 = phonon_ref.supercell(basis + rng.normal(0.0, rattle, basis.shape), C, reps)
        assert np.array_equal(S, S2)
        brute, margin = phonon_ref.images_brute(pos_sc, S, 2)
        assert margin > 1e-9, margin
        _, _, kept = phonon_ref.images_27(pos_sc, S, np.linalg.inv(S), 2)
        assert {k: sorted(v) for k, v in kept.items()} == brute
        if rattle == 0.0 and max(reps) == 2 and min(reps) == 2:
            assert max(len(v) for v in brute.values()) >= 2   # ties exist


# ------------------------------------------------------------------------------------------------ validation
def test_validation_names_the_system():
    from sevennet_amd.phonon import validate_phonon_inputs
    ok = dict(n_atoms=[2, 1], cells=np.stack([CUBIC, FCC]), pbcs=np.ones((2, 3), bool), supercells=(2, 2, 2), qpoints=np.zeros((1, 3)),
              mesh=(2, 2, 2), temperatures=[0.0, 300.0], symprec=1e-5, e_min=1e-5, dos_bins=20, max_q_per_call=8)

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            validate_phonon_inputs(**dict(ok, **kw))

    reps, q, mesh, T = validate_phonon_inputs(**ok)
    assert reps.tolist() == [[2, 2, 2], [2, 2, 2]] and len(q) == 2 and mesh == (2, 2, 2) and T.tolist() == [0.0, 300.0]
    reps, q, mesh, T = validate_phonon_inputs(**dict(ok, supercells=[(1, 2, 3), (2, 2, 2)], qpoints=[np.zeros((2, 3)), np.ones((1, 3))],
                                                     mesh=None, temperatures=None))
    assert reps.tolist() == [[1, 2, 3], [2, 2, 2]] and [len(x) for x in q] == [2, 1] and mesh is None and len(T) == 0
    for s in ((0, 1, 1), (1, 1), (1.5, 1, 1), (True, True, True), [(1, 1, 1)] * 3):
        bad('supercell', supercells=s)
    bad('system 1: supercell', supercells=[(1, 1, 1), (1, -1, 1)])
    bad('system 1: phonons need a fully periodic system', pbcs=np.array([[True] * 3, [True, True, False]]))
    sheared = CUBIC.copy()
    sheared[2] += 2.0 * sheared[0]
    bad('system 0: the supercell .* is not reduced', cells=np.stack([sheared, FCC]))
    bad('system 1: the cell is singular', cells=np.stack([CUBIC, np.zeros((3, 3))]))
    bad('pass `qpoints`, `mesh` or both', qpoints=None, mesh=None, temperatures=None)
    bad('qpoints: None, one', qpoints=np.zeros(3))
    bad('system 1: q-points are a finite', qpoints=[np.zeros((1, 3)), np.zeros((2, 2))])
    bad('system 0: q-points are a finite', qpoints=[np.full((1, 3), np.nan), np.zeros((2, 3))])
    bad('system 1: no q-point is given', qpoints=[np.zeros((1, 3)), np.zeros((0, 3))], mesh=None, temperatures=None)
    for mesh in ((0, 1, 1), (2, 2), 4, (1.0, 1.0, 1.0)):
        bad('mesh', mesh=mesh)
    bad('temperatures need a `mesh`', mesh=None)
    for T in ([-1.0], [np.nan], [[1.0]]):
        bad('temperatures', temperatures=T)
    for v in (-1e-5, float('nan'), None, 'x'):
        bad('symprec', symprec=v)
        bad('e_min', e_min=v)
    for bins in (0, -3, [1.0], [0.0, 0.0, 1.0], [0.0, np.inf], True, 2.5):
        bad('dos_bins', dos_bins=bins)
    for c in (0, 2.5, None, True):
        bad('max_q_per_call', max_q_per_call=c)
    validate_phonon_inputs(**dict(ok, dos_bins=[0.0, 0.01, 0.05]))


# ------------------------------------------------------------------------------------------------ thermodynamics, dos, path
def test_thermodynamics_of_a_single_frequency_is_einsteins():
    from sevennet_amd.md import KB
    from sevennet_amd.phonon import thermodynamics
    hv, T = 0.031, np.array([0.0, 50.0, 300.0, 2000.0])
    got = thermodynamics(np.full((4, 3), hv), T)   # four mesh points, three equal modes each
    x = hv / (KB * T[1:])
    assert abs(got['zpe'] - 1.5 * hv) <= 1e-15 and got['n_imaginary'] == 0 and got['n_skipped'] == 0
    assert got['free_energy'][0] == got['zpe'] and got['entropy'][0] == 0.0 and got['heat_capacity'][0] == 0.0   # the T = 0 branch
    einstein = dict(free_energy=3 * (hv / 2 + KB * T[1:] * np.log(1 - np.exp(-x))),
                    entropy=3 * KB * (x / (np.exp(x) - 1) - np.log(1 - np.exp(-x))),
                    heat_capacity=3 * KB * x ** 2 * np.exp(x) / (np.exp(x) - 1) ** 2)
    ref = phonon_ref.thermodynamics(np.full((4, 3), hv), T)
    for key, want in einstein.items():   # (1e-12 relative: e^x - 1 and 1 - e^-x lose a few digits at x = 0.18, the smallest here)
        assert (np.abs(got[key][1:] - want) <= 1e-12 * np.abs(want)).all(), key
        assert (np.abs(got[key] - ref[key]) <= 1e-12 * np.abs(ref[key])).all(), key
    # very cold: e^x overflows a naive formula, the sums stay finite and go to the T = 0 values
    cold = thermodynamics(np.full((1, 3), hv), [0.1])
    assert np.isfinite(cold['heat_capacity']).all() and cold['heat_capacity'][0] < 1e-300 and abs(cold['free_energy'][0] - 1.5 * hv) <= 1e-15


def test_heat_capacity_goes_to_dulong_petit():
    """C_v / k_B per mode = 1 - x^2 / 12 + x^4 / 240 - ...: within x^4 of 1 - x^2 / 12 at small x"""
    from sevennet_amd.md import KB
    from sevennet_amd.phonon import thermodynamics
    hv = 0.01
    for x in (0.3, 0.1, 0.01):
        c = thermodynamics([[hv]], [hv / (KB * x)])['heat_capacity'][0] / KB
        assert abs(c - (1.0 - x * x / 12.0)) <= x ** 4, (x, c)


def test_imaginary_and_skipped_modes_are_counted_and_left_out():
    from sevennet_amd.phonon import thermodynamics
    e = np.array([[-0.02, 0.0, 5e-6, 0.03], [-1e-6, 1e-5, 0.03, 0.03]])   # (1e-5 itself is skipped: h nu > e_min is required)
    got = thermodynamics(e, [0.0, 300.0], e_min=1e-5)
    only = thermodynamics(np.array([[0.03, 0.0, 0.0], [0.03, 0.03, 0.0]]), [0.0, 300.0])   # the three modes that count, in the same order
    assert got['n_imaginary'] == 1 and got['n_skipped'] == 4
    assert abs(got['zpe'] - 0.5 * 0.09 / 2) <= 1e-16
    for key in ('free_energy', 'entropy', 'heat_capacity'):
        assert np.array_equal(got[key], only[key]), key
    nan = thermodynamics(np.full((2, 3), np.nan), [10.0])
    assert np.isnan(nan['free_energy']).all() and np.isnan(nan['zpe'])


def test_band_path_and_dos():
    from sevennet_amd.phonon import band_path, dos, mesh_points
    path = band_path([[0, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0]], 4)
    assert path.shape == (9, 3) and np.array_equal(path[0], [0, 0, 0]) and np.array_equal(path[4], [0.5, 0, 0]) and np.array_equal(path[8], [0.5, 0.5, 0])
    assert np.allclose(path[1], [0.125, 0, 0], atol=0, rtol=1e-15) and np.allclose(path[6], [0.5, 0.25, 0], atol=0, rtol=1e-15)
    for pts, n in (([[0, 0, 0]], 2), ([[0, 0], [1, 1]], 2), ([[0, 0, 0], [1, 1, 1]], 0), ([[0, 0, 0], [1, 1, 1]], 1.5)):
        with pytest.raises(ValueError, match='band_path'):
            band_path(pts, n)
    mp = mesh_points((2, 1, 3))
    assert mp.shape == (6, 3) and np.array_equal(mp[0], [0, 0, 0]) and np.array_equal(mp[1], [0, 0, 1 / 3]) and np.array_equal(mp[3], [0.5, 0, 0])
    rng = np.random.default_rng(1)
    e = rng.uniform(-0.01, 0.08, (24, 6))   # 24 mesh points, 3m = 6
    centres, density = dos(e, 50)
    width = centres[1] - centres[0]
    assert centres.shape == density.shape == (50,) and abs((density * width).sum() - 6.0) <= 1e-12
    edges = np.array([0.0, 0.02, 0.05, 0.1])
    centres, density = dos(e, edges)
    assert np.allclose(centres, [0.01, 0.035, 0.075], atol=0, rtol=1e-15)
    assert abs((density * np.diff(edges)).sum() - (e >= 0).sum() / 24) <= 1e-12    # the modes below the first edge are outside
    c_nan, d_nan = dos(np.full((2, 3), np.nan), 7)
    assert c_nan.shape == (7,) and np.isnan(d_nan).all()


def test_driver_constants_are_the_restatements():
    from sevennet_amd import md, phonon
    assert phonon.KB == md.KB == phonon_ref.KB and phonon.HBAR == vib_ref.HBAR and phonon.ACC == vib_ref.ACC
    pos, cell, _ = phonon_ref.chain_cell()
    t, p, S = phonon.build_supercell([0, 1], pos, cell, (2, 1, 3))
    p_ref, S_ref = phonon_ref.supercell(pos, cell, (2, 1, 3))
    assert np.array_equal(p, p_ref) and np.array_equal(S, S_ref) and t.tolist() == [0, 1] * 6
    assert np.array_equal(phonon_ref.q_cartesian([[0.1, 0.2, 0.3]], HEX)[0], 2.0 * np.pi * (np.array([0.1, 0.2, 0.3]) @ np.linalg.inv(HEX).T))
    rng = np.random.default_rng(3)
    M = rng.normal(size=(2, 6, 6)) + 1j * rng.normal(size=(2, 6, 6))
    D = (M + np.conj(np.swapaxes(M, 1, 2))) * 0.5
    sp = phonon.spectrum(D, want_modes=True)
    assert sp['modes'].shape == (2, 6, 2, 3) and np.array_equal(sp['energies'], phonon_ref.energies_of(sp['eigenvalues']))
    v = sp['modes'][1, 4].reshape(6)
    assert np.abs(D[1] @ v - sp['eigenvalues'][1, 4] * v).max() <= 1e-12 * np.abs(D).max() * 6
    bad = phonon.spectrum(np.full((2, 3, 3), np.nan + 0j))
    assert np.isnan(bad['energies']).all() and bad['energies'].shape == (2, 3)
