"""CPU: the fp64 restatement of the nudged-elastic-band rule (neb_ref) finds a saddle point that is known in closed form, takes
every branch of the improved tangent where it should, and the host side of sevennet_amd.neb (interpolation, minimum image,
argument validation, the ABI entry) does what it says without a device."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import neb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPEN = (np.zeros((3, 3)), [False] * 3)
FMAX = 1e-3


def _relax(n, m, climb, seed=0):
    return neb_ref.neb_relax(neb_ref.saddle_band(n, m, seed), neb_ref.saddle_potential, *OPEN, fmax=FMAX, steps=400, k=0.1, climb=climb)


def test_the_potential_is_what_its_docstring_says():
    e, f = neb_ref.saddle_potential([[-1.0, 0, 0], [1.0, 0, 0], [0.0, neb_ref.SADDLE_A, 0.0]])
    assert e == 1.0 and np.array_equal(f, np.zeros((3, 3)))
    rng = np.random.default_rng(0)
    p = rng.normal(0, 0.7, (4, 3))
    h = 1e-6
    for i in range(4):
        for c in range(3):
            d = np.zeros_like(p)
            d[i, c] = h
            num = -(neb_ref.saddle_potential(p + d)[0] - neb_ref.saddle_potential(p - d)[0]) / (2 * h)
            assert abs(num - neb_ref.saddle_potential(p)[1][i, c]) < 1e-7
    # the Hessian at the saddle: d2V/dx2 = -4 + 0 (u = 0 there, and du/dx = 0 at x = 0), d2V/dy2 = 4, d2V/dz2 = 4
    s = np.array([[0.0, neb_ref.SADDLE_A, 0.0]])
    curv = [-(neb_ref.saddle_potential(s + h * np.eye(3)[c])[1][0, c] - neb_ref.saddle_potential(s - h * np.eye(3)[c])[1][0, c]) / (2 * h)
            for c in range(3)]
    assert np.allclose(curv, [-4.0, 4.0, 4.0], atol=1e-6)


@pytest.mark.parametrize('n,m', [(1, 5), (3, 5), (3, 4), (7, 3), (3, 1)])
def test_climbing_band_finds_the_known_saddle(n, m):
    """barrier 1 within n fmax^2 / 4: every atom of the climbing image has |F| < fmax at convergence (the climbing image's NEB
    force has the length of its true force), the smallest |curvature| at the saddle is 4, so the harmonic energy error is at most
    n fmax^2 / 8; doubled for the anharmonic remainder"""
    r = _relax(n, m, climb=True)
    assert r['converged'], r['n_steps']
    barrier = r['energies'].max() - r['energies'][0]
    top = r['images'][1 + r['imax'], 0]
    print(f'(n, m) = ({n}, {m}): converged after {r["n_steps"]} steps, |barrier - 1| = {abs(barrier - 1):.2e}, climbing image at {top}')
    assert abs(barrier - 1.0) <= n * FMAX ** 2 / 4
    assert abs(top[0]) < 1e-3 and abs(top[1] - neb_ref.SADDLE_A) < 1e-3 and abs(top[2]) < 1e-3


def test_without_climbing_an_even_band_misses_the_saddle():
    r = _relax(3, 4, climb=False)
    assert r['converged']
    barrier = r['energies'].max() - r['energies'][0]
    print(f'plain band (3, 4): barrier {barrier:.4f}')
    assert barrier < 0.95


def _three(tp, tm):
    """a three-image band of one atom with t- = tm and t+ = tp around the origin"""
    return np.array([[-np.asarray(tm, float)], [[0.0, 0.0, 0.0]], [np.asarray(tp, float)]])


@pytest.mark.parametrize('energies,branch,want', [
    ((0.0, 1.0, 2.0), 'rising', 'tp'),
    ((2.0, 1.0, 0.0), 'falling', 'tm'),
    ((0.0, 2.0, 1.5), 'maximum_up', (2.0, 0.5)),      # Ep > Em: t+ dmax + t- dmin, dmax = |Em - Ei| = 2, dmin = 0.5
    ((1.5, 2.0, 0.0), 'maximum_down', (0.5, 2.0)),    # Ep < Em: t+ dmin + t- dmax
    ((3.0, 1.0, 2.0), 'minimum_down', (1.0, 2.0)),    # a minimum with Ep < Em
    ((1.0, 2.0, 1.0), 'maximum_tie', (1.0, 1.0)),     # the exact tie lands in the else branch
])
def test_tangent_branches(energies, branch, want):
    tp, tm = np.array([0.3, 0.4, 0.0]), np.array([0.0, 0.5, 0.2])
    band = _three(tp, tm)
    F = np.array([[0.7, -0.2, 0.4]])
    f, imax, info = neb_ref.neb_forces(band, F[None], energies, *OPEN, k=0.3)
    assert info[0]['branch'] == branch and imax == 0
    tau = tp if want == 'tp' else tm if want == 'tm' else want[0] * tp + want[1] * tm
    tau = tau / np.linalg.norm(tau)
    expect = F[0] - (F[0] @ tau) * tau + 0.3 * (np.linalg.norm(tp) - np.linalg.norm(tm)) * tau
    assert np.allclose(f[0, 0], expect, rtol=0, atol=1e-15)
    climbed, _, _ = neb_ref.neb_forces(band, F[None], energies, *OPEN, k=0.3, climb=True)
    assert np.allclose(climbed[0, 0], F[0] - 2 * (F[0] @ tau) * tau, rtol=0, atol=1e-15)   # one interior image: it climbs


def test_zero_tangent_leaves_the_force_alone():
    band = np.zeros((3, 2, 3))
    F = np.array([[[1.0, 2.0, 3.0], [-1.0, 0.5, 0.0]]])
    f, _, info = neb_ref.neb_forces(band, F, (0.0, 1.0, 0.0), *OPEN, k=0.1)
    assert info[0]['branch'] == 'zero' and np.array_equal(f, F)


def test_mic_across_a_triclinic_face_and_with_an_open_axis():
    from sevennet_amd import neb
    cell = np.array([[4.0, 0.0, 0.0], [1.0, 5.0, 0.0], [0.5, -0.7, 6.0]])
    rng = np.random.default_rng(1)
    for mod, pbc in ((neb_ref, [True] * 3), (neb, [True] * 3), (neb_ref, [True, True, False]), (neb, [True, True, False])):
        d = rng.normal(0, 0.4, (50, 3))                       # shorter than half the smallest height (2)
        shift = rng.integers(-2, 3, (50, 3)).astype(float)
        shift[:, ~np.asarray(pbc)] = 0.0
        got = mod.mic(d + shift @ cell, cell, pbc)
        assert np.abs(got - d).max() < 1e-13
    # an open axis is not wrapped, whatever its length; its zero cell row is padded
    slab = np.array([[4.0, 0, 0], [0, 4.0, 0], [0, 0, 0]])
    for mod in (neb_ref, neb):
        got = mod.mic(np.array([[3.5, -3.9, 17.0]]), slab, [True, True, False])
        assert np.allclose(got, [[-0.5, 0.1, 17.0]], atol=1e-14)
        d = np.array([[30.0, -40.0, 50.0]])
        assert np.array_equal(mod.mic(d, np.zeros((3, 3)), [False] * 3), d)   # no periodic axis: the bits are kept
    # in a band: an image pair that straddles a face has the short tangent
    a, b = np.array([[0.2, 0.1, 0.1]]), np.array([[-0.2, 0.1, 0.1]]) + cell[0]
    band = np.array([a, b, b + [0.3, 0, 0]])
    _, _, info = neb_ref.neb_forces(band, np.zeros((1, 1, 3)), (0.0, 1.0, 2.0), cell, [True] * 3, k=0.1)
    assert abs(info[0]['tm'] - 0.4) < 1e-13 and abs(info[0]['tp'] - 0.3) < 1e-13


def test_fixed_atoms_get_zero_neb_force():
    rng = np.random.default_rng(2)
    band = rng.normal(0, 0.3, (5, 6, 3))
    F = rng.normal(0, 1.0, (3, 6, 3))
    E = [0.0, 0.4, 0.9, 0.5, 0.1]
    for fixed in ([1, 4], np.array([False, True, False, False, True, False])):
        for climb in (False, True):
            f, _, _ = neb_ref.neb_forces(band, F, E, *OPEN, k=0.1, climb=climb, fixed=fixed)
            assert np.array_equal(f[:, [1, 4]], np.zeros((3, 2, 3))) and (np.abs(f[:, [0, 2, 3, 5]]).min(axis=(0, 2)) > 0).all()
    # a fixed atom's true force does not enter F . tau
    F2 = F.copy()
    F2[:, [1, 4]] += 5.0
    a, _, _ = neb_ref.neb_forces(band, F, E, *OPEN, k=0.1, fixed=[1, 4])
    b, _, _ = neb_ref.neb_forces(band, F2, E, *OPEN, k=0.1, fixed=[1, 4])
    assert np.array_equal(a, b)


def test_interpolate_band():
    from sevennet_amd.neb import interpolate_band
    rng = np.random.default_rng(3)
    cell = np.array([[4.0, 0.0, 0.0], [1.0, 5.0, 0.0], [0.5, -0.7, 6.0]])
    a = rng.uniform(0, 1, (7, 3)) @ cell
    b = a + rng.normal(0, 0.1, (7, 3))
    b[2] = a[2] - 0.3 * cell[0] / 4.0 + cell[0]    # atom 2 leaves through the face at x = 0 and is given wrapped back in
    band = interpolate_band(a, b, 6, cell, [True] * 3)
    assert band.shape == (6, 7, 3) and np.array_equal(band[0], a) and np.array_equal(band[-1], b)   # bit for bit
    steps = np.linalg.norm(band[1:-1, 2] - band[:-2, 2], axis=1)
    assert np.allclose(steps, 0.3 / 5, atol=1e-13)   # the short way, in equal steps (the last image is the caller's, a cell away)
    plain = interpolate_band(a, b, 6)
    assert np.allclose(plain[1], a + (b - a) / 5, atol=1e-15) and np.array_equal(plain[-1], b)
    with pytest.raises(ValueError, match='endpoints of shape'):
        interpolate_band(a, b[:3], 5)
    with pytest.raises(ValueError, match='n_images = 1'):
        interpolate_band(a, b, 1)


def test_neb_batch_refuses_bad_input_before_any_device_work():
    from sevennet_amd.neb import neb_batch
    engine = SimpleNamespace(spec=SimpleNamespace(num_species=2))   # (no `dev`: anything that reached the device would fail on it)
    types, band = [np.array([0, 1, 0])], np.zeros((4, 3, 3)) + np.arange(4)[:, None, None]
    cell, pbc = np.eye(3)[None] * 6.0, [True] * 3

    def call(match, types_list=types, images_list=None, cells=cell, pbcs=pbc, **kw):
        with pytest.raises(ValueError, match=match):
            neb_batch(engine, types_list, [band] if images_list is None else images_list, cells, pbcs, cutoff=4.0, **kw)

    call('band 0: 2 images, but a band needs two endpoints', images_list=[band[:2]])
    call(r'band 1: images of shape \[M,n,3\] are required, got \(4, 3\)', types_list=types * 2, images_list=[band, band[:, :, 0]],
         cells=np.concatenate([cell, cell]))
    call('band 0: 3 species but images of 2 atoms', images_list=[band[:, :2]])
    call('1 species arrays but 2 bands', images_list=[band, band], cells=np.concatenate([cell, cell]))
    call('1 bands but cells of shape', cells=np.zeros((2, 3, 3)))
    call('1 bands but pbc of shape', pbcs=np.zeros((2, 3), bool))
    call('band 0: spring constant k = 0.0', k=0.0)
    call('band 0: spring constant k = -1.0', k=-1.0)
    call('band 0: spring constant k = nan', k=float('nan'))
    call('band 0: spring constant k = inf', k=[float('inf')])
    call(r'k: one spring constant, or one per band \(1\), is required, got 2', k=[0.1, 0.2])
    call('band 0: fixed atom index 3 is out of range', fixed_list=[[0, 3]])
    call('band 0: fixed atom index -1 is out of range', fixed_list=[[-1]])
    call(r'band 0: a fixed mask of shape \(3,\) is required', fixed_list=[np.array([True, False])])
    call('fixed_list has 2 entries but there are 1 bands', fixed_list=[None, None])
    call('band 0: singular cell', cells=np.zeros((1, 3, 3)))
    call('unknown species index 2', types_list=[np.array([0, 2, 0])])
    call('non-finite position', images_list=[np.where(np.arange(4)[:, None, None] == 2, np.nan, band)])
    call("unknown FIRE parameter 'dt'", dt=0.1)
    call('fmax = -1', fmax=-1.0)
    call('steps = 1.5', steps=1.5)


def test_abi_entry():
    from sevennet_amd import _lib
    assert _lib.ABI_VERSION == 4
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'snet_hip.h')).read(), flags=re.S)
    args = re.search(r'\bint snet_neb_forces\s*\((.*?)\)\s*;', text, flags=re.S).group(1)
    assert len(_lib.SIGNATURES['snet_neb_forces'][1]) == len(args.split(',')) == 25
    assert 'snet_neb.hip' in __import__('sevennet_amd.build', fromlist=['STATIC_SOURCES']).STATIC_SOURCES
    assert hasattr(_lib.load(), 'snet_neb_forces')
