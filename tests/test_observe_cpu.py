"""CPU: the MD observables -- the fp64 restatement (observe_ref) against known answers, the ring bookkeeping as a pure host
function, the host helpers, every input check of the driver (before any device work) and the binding of the two entry points."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import observe_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
def test_fcc_coordination_shells_from_the_conventional_cell():
    """fcc, a = 4, four atoms: shells at a/sqrt(2), a, a sqrt(3/2), a sqrt(2) hold 12, 6, 24, 12 neighbours.  r_max = 6 is above
    the cell height 4, so an atom's own images count (the shell at a consists of nothing else); 60 bins of 0.1 A put the shell
    radii 2.828, 4, 4.899, 5.657 at least 0.028 A from an edge -- except a = 4.0 itself, so the bins are 0.09 A: 66 of them"""
    a = 4.0
    pos = a * np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    pos = pos + np.array([3 * a, -2 * a, a]) * np.array([[1], [0], [2], [-1]])   # whole cells away: must not matter
    bins, dr = 66, 0.09
    counts, margin = ref.rdf_counts(pos, np.zeros(4, int), 1, np.eye(3) * a, [True] * 3, bins * dr, bins)
    assert margin > 0.01
    shells = {int(r / dr): n for r, n in ((a / np.sqrt(2), 12), (a, 6), (a * np.sqrt(1.5), 24), (a * np.sqrt(2), 12))}
    want = np.zeros(bins, np.int64)
    for b, n in shells.items():
        want[b] = 4 * n
    assert counts.shape == (1, 1, bins) and np.array_equal(counts[0, 0], want)
    two, _ = ref.rdf_counts(pos, np.array([0, 1, 1, 1]), 2, np.eye(3) * a, [True] * 3, bins * dr, bins)
    assert np.array_equal(two.sum((0, 1)), want) and np.array_equal(two[0, 1], two[1, 0])
    first = int(a / np.sqrt(2) / dr)
    assert two[0, 0, first] == 0 and two[0, 1, first] == 12 and two[1, 1, first] == 24 and two[0, 0, int(a / dr)] == 6


def test_g_of_uniform_random_points_is_one():
    """2 000 uniform points in a cube of 20 A, 10 bins to 5 A: counts[bin] is close to Poisson with mean N (N/V) shell, so g scatters by
    1 / sqrt(mean) (ordered pairs count every pair twice: sqrt(2) of that); five of those"""
    n, L, bins, r_max = 2000, 20.0, 10, 5.0
    pos = np.random.default_rng(0).uniform(0, L, (n, 3))
    counts, _ = ref.rdf_counts(pos, np.zeros(n, int), 1, np.eye(3) * L, [True] * 3, r_max, bins)
    edges = np.linspace(0, r_max, bins + 1)
    mean = n * (n / L ** 3) * 4 / 3 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    g = counts[0, 0] / mean
    assert (np.abs(g - 1) <= 5 * np.sqrt(2 / mean)).all(), g


def test_open_axes_and_molecules():
    """a slab repeats along x and y only; a molecule has the plain pair distances"""
    pos = np.array([[0.1, 0.2, 0.0], [0.1, 0.2, 7.5]])
    slab, _ = ref.rdf_counts(pos, [0, 0], 1, np.diag([3.0, 3.0, 0.0]), [True, True, False], 4.0, 8)
    assert slab[0, 0].tolist() == [0, 0, 0, 0, 0, 0, 8, 0]            # four images at 3.0 each, none across z
    mol, margin = ref.rdf_counts(pos, [0, 1], 2, np.zeros((3, 3)), [False] * 3, 10.0, 10)
    assert mol.sum() == 2 and mol[0, 1, 7] == 1 and mol[1, 0, 7] == 1 and margin == pytest.approx(0.5)


def test_ballistic_msd_and_vacf():
    """x(t) = x0 + v t per atom: d_i = v_i l dt, so msd_sum[l] = n_origins[l] sum |v|^2 (l dt)^2 and vacf_sum[l] = n_origins[l] sum |v|^2"""
    rng = np.random.default_rng(1)
    n, T, dt, lags, oe = 6, 11, 0.5, 4, 3
    v = rng.normal(0, 1, (n, 3))
    pos = rng.normal(0, 1, (n, 3))[None] + v[None] * (np.arange(T) * dt)[:, None, None]
    vel = np.broadcast_to(v, (T, n, 3))
    kind = np.array([0, 0, 1, 1, 1, 0])
    msd, vacf, n_or = ref.correlate(pos, vel, np.ones(n), kind, 2, lags, oe, remove_com=False)
    assert n_or.tolist() == [4, 4, 3, 3]                               # origins 0 3 6 9; 9 + 2 is past the end
    for k in range(2):
        v2 = (v[kind == k] ** 2).sum()
        assert np.allclose(msd[k], n_or * v2 * (np.arange(lags) * dt) ** 2, rtol=1e-12, atol=1e-13)
        assert np.allclose(vacf[k], n_or * v2, rtol=1e-12)
    drift = pos + np.array([0.3, -0.2, 0.1]) * (np.arange(T) * dt)[:, None, None]    # a common drift goes with remove_com
    a = ref.correlate(drift, vel + np.array([0.3, -0.2, 0.1]), np.ones(n), kind, 2, lags, oe)
    b = ref.correlate(pos, vel, np.ones(n), kind, 2, lags, oe)
    assert np.allclose(a[0], b[0], rtol=1e-10, atol=1e-12) and np.allclose(a[1], b[1], rtol=1e-10)
    one = ref.correlate(pos[:, :1], vel[:, :1], np.ones(1), [0], 1, lags, oe)
    assert not one[0].any() and not one[1].any() and one[2].tolist() == n_or.tolist()


# ------------------------------------------------------------------------------------------------ the ring
@pytest.mark.parametrize('steps, every, lags, origin_every', [(40, 1, 7, 3), (39, 2, 7, 3), (12, 2, 3, 1), (12, 5, 4, 2), (7, 3, 9, 4),
                                                              (0, 1, 3, 2), (25, 1, 6, 6), (25, 1, 5, 7)])
def test_ring_bookkeeping(steps, every, lags, origin_every):
    """slot and lag of every live origin, sample by sample, against a list of (origin sample -> slot) kept by hand; and n_origins
    against the restatement's double loop"""
    from sevennet_amd.observe import live_origins, origin_counts, ring_size
    n_samples = steps // every + 1
    R = ring_size(lags, origin_every)
    assert (R - 1) * origin_every < lags <= R * origin_every
    slots, seen = {}, np.zeros(lags, np.int64)
    for s in range(n_samples):
        if s % origin_every == 0:
            slots[(s // origin_every) % R] = s            # the copy the driver makes before the launch
        live = live_origins(s, lags, origin_every)
        want = sorted((slot, s - so) for slot, so in slots.items() if s - so < lags)
        assert sorted(live) == want, (s, live, want)
        assert len({lag for _, lag in live}) == len(live)   # distinct lags: no two workgroups write one slot
        for _, lag in live:
            seen[lag] += 1
    assert np.array_equal(origin_counts(n_samples, lags, origin_every), seen)
    z = np.zeros((n_samples, 1, 3))
    assert np.array_equal(ref.correlate(z, z, np.ones(1), [0], 1, lags, origin_every)[2], seen)


# ------------------------------------------------------------------------------------------------ host helpers
def test_diffusion_coefficient_of_a_linear_msd():
    from sevennet_amd.observe import diffusion_coefficient
    t = np.arange(50) * 2.0
    D, res = diffusion_coefficient(6 * 0.0123 * t + 0.4, t, fit=(10.0, 80.0))
    assert D == pytest.approx(0.0123, rel=1e-12) and res <= 1e-12
    msd = 6 * 0.0123 * t + 0.4
    msd[:5] = 0.01 * t[:5] ** 2                                        # a ballistic start outside the window changes nothing
    assert diffusion_coefficient(msd, t, fit=(10.0, 80.0))[0] == pytest.approx(0.0123, rel=1e-12)
    assert diffusion_coefficient(msd, t, fit=(0.0, 80.0))[1] > 1e-3
    with pytest.raises(ValueError, match='fewer than two'):
        diffusion_coefficient(msd, t, fit=(10.5, 11.5))


def test_vdos_of_a_cosine_peaks_at_its_frequency():
    from sevennet_amd.observe import LIGHT_CM_PER_FS, vdos
    dt, n = 2.0, 400
    f0 = 0.0125                                                        # 1/fs: 80 fs period, 417 1/cm
    nu, spec = vdos(np.cos(2 * np.pi * f0 * np.arange(n) * dt), dt)
    assert nu[0] == 0.0 and nu[-1] == pytest.approx(1 / (2 * dt) / LIGHT_CM_PER_FS) and len(nu) == len(spec) == n
    assert abs(nu[np.argmax(spec)] - f0 / LIGHT_CM_PER_FS) <= nu[1]       # within one step of the frequency grid
    assert spec.max() == pytest.approx(n * dt, rel=0.02)               # int_0^T cos^2 = T / 2, times 2
    fine = vdos(np.cos(2 * np.pi * f0 * np.arange(n) * dt), dt, n_freq=4000)
    assert abs(fine[0][np.argmax(fine[1])] - f0 / LIGHT_CM_PER_FS) <= fine[0][1]


# ------------------------------------------------------------------------------------------------ inputs
class _NoDeviceEngine:
    spec = SimpleNamespace(num_species=12)

    def __getattr__(self, name):
        raise AssertionError(f'the engine was touched ({name}) before the input was validated')


@pytest.fixture
def no_device(monkeypatch):
    """the library cannot be loaded and torch.cuda may not be touched"""
    import torch
    from sevennet_amd import _lib

    def no_library():
        raise AssertionError('the library was loaded before the input was validated')

    def touched(*a, **k):
        raise AssertionError('torch.cuda was touched before the input was validated')
    monkeypatch.setattr(_lib, 'load', no_library)
    for name in ('device', 'current_stream', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, touched)


def _md(observe, **kw):
    from sevennet_amd.md import md_batch
    args = dict(types=[np.array([0, 1]), np.arange(9)], positions=[np.array([[0.0, 0, 0], [1.2, 0, 0]]), np.arange(27.0).reshape(9, 3) / 5],
                masses=[np.array([28.0, 16.0]), np.full(9, 12.0)], cells=np.stack([np.eye(3) * 6.0, np.diag([6.0, 6.0, 1.0])]),
                pbcs=np.ones((2, 3), bool), cutoff=5.0, dt=1.0, steps=3, temperature=300.0, observe=observe)
    args.update(kw)
    return md_batch(_NoDeviceEngine(), args.pop('types'), args.pop('positions'), args.pop('masses'), args.pop('cells'),
                    args.pop('pbcs'), **args)


def _bad_inputs():
    from sevennet_amd.observe import Observe
    nine = dict(types=[np.array([0, 1]), np.zeros(9, int)])
    return [
        (Observe(every=0, lags=2), nine, 'every = 0'),
        (Observe(every=1.5, lags=2), nine, 'every = 1.5'),
        (Observe(every=True, lags=2), nine, 'every = True'),
        (Observe(every=1, rdf_rmax=0.0), nine, 'rdf_rmax = 0.0'),
        (Observe(every=1, rdf_rmax=-1.0), nine, 'rdf_rmax'),
        (Observe(every=1, rdf_rmax=float('inf')), nine, 'rdf_rmax'),
        (Observe(every=1, rdf_rmax=float('nan')), nine, 'rdf_rmax'),
        (Observe(every=1, rdf_rmax=2.0, rdf_bins=0), nine, 'rdf_bins = 0'),
        (Observe(every=1, lags=-1), nine, 'lags = -1'),
        (Observe(every=1, lags=3, origin_every=0), nine, 'origin_every = 0'),
        (Observe(every=1), nine, 'nothing to accumulate'),
        (Observe(every=1, lags=70000), nine, 'ring of 70000'),
        ('rdf', nine, 'observe.Observe is required'),
        (Observe(every=1, lags=2), {}, 'system 1: 9 species'),                       # more than 8 kinds
        (Observe(every=1, rdf_rmax=2.0, rdf_bins=2049), nine, 'system 0: 2 kinds and 2049 bins'),   # 4 x 2049 > 8192
        (Observe(every=1, rdf_rmax=4.6), nine, 'system 1: .*5 cells along axis 2.*use a supercell'),   # floor(4.6 / 1 + 0.5) = 5
        (Observe(every=1, lags=2), dict(pressure=0.01, compressibility=50.0, types=nine['types']), 'observe with pressure'),
    ]


@pytest.mark.parametrize('case', range(17))
def test_bad_observe_input_raises_before_any_device_work(no_device, case):
    observe, kw, match = _bad_inputs()[case]
    with pytest.raises(ValueError, match=match):
        _md(observe, **kw)


def test_caps_are_at_their_stated_values(no_device):
    """what just passes the three caps: 8 kinds, kinds^2 bins == 8192, reach 4; by_species=False folds nine species into one kind"""
    from sevennet_amd.observe import MAX_HIST, MAX_KINDS, MAX_REACH, Observe, image_reach, observe_plan
    assert (MAX_KINDS, MAX_HIST, MAX_REACH) == (8, 8192, 4) and len(_bad_inputs()) == 17
    n_at = np.array([2, 9])
    cells, pbcs = np.stack([np.eye(3) * 6.0, np.diag([6.0, 6.0, 1.0])]), np.ones((2, 3), bool)
    types = np.concatenate([[0, 1], np.arange(8), [3]])
    plan = observe_plan(Observe(every=1, rdf_rmax=4.4, rdf_bins=128, lags=3), types, n_at, cells, pbcs)   # 64 x 128 = 8192
    assert plan['n_kinds'].tolist() == [2, 8] and plan['kind'].tolist() == [0, 1, 0, 1, 2, 3, 4, 5, 6, 7, 3]
    assert plan['kind_ptr'].tolist() == [0, 2, 10] and plan['count_ptr'].tolist() == [0, 512, 512 + 8192]
    assert plan['sys_desc'].tolist() == [[2, 0, 7, 1, 1, 1, 0, 0], [8, 512, 7, 1, 1, 4, 0, 0]]       # floor(4.4 / 6 + 0.5) = 1
    assert plan['tile'].tolist() == [[0, 0, 2], [1, 0, 9]] and plan['kinds_max'] == 8 and plan['reach_max'] == 4
    folded = observe_plan(Observe(every=1, lags=2, by_species=False), np.arange(11), n_at, cells, pbcs)
    assert folded['n_kinds'].tolist() == [1, 1] and not folded['kind'].any() and folded['kinds'] == [None, None]
    # reach: per axis, by the face-to-face height (triclinic: 60 degrees between a and b), 0 on an open axis
    tri = np.array([[4.0, 0, 0], [2.0, 2 * np.sqrt(3), 0], [0, 0, 0]])
    reach = image_reach(tri[None], np.array([[True, True, False]]), 5.0)
    assert reach.tolist() == [[int(np.floor(5.0 / (2 * np.sqrt(3)) + 0.5))] * 2 + [0]] == [[1, 1, 0]]
    assert plan_tiles(70) == [[0, 0, 32], [0, 32, 32], [0, 64, 6]]


def plan_tiles(n):
    from sevennet_amd.observe import Observe, observe_plan
    p = observe_plan(Observe(every=1, rdf_rmax=2.0, rdf_bins=4), np.zeros(n, int), np.array([n]), np.eye(3)[None] * 9.0, np.ones((1, 3), bool))
    return p['tile'].tolist()


def test_attach_observables_normalisation():
    """g, msd and vacf from hand-made accumulators: the divisions of the documentation, NaN where a lag has no origin"""
    from sevennet_amd.observe import Observe, attach_observables, observe_plan
    obs = Observe(every=2, rdf_rmax=2.0, rdf_bins=4, lags=3, origin_every=2)
    cells, pbcs = np.stack([np.eye(3) * 5.0, np.zeros((3, 3))]), np.array([[True] * 3, [False] * 3])
    plan = observe_plan(obs, np.array([1, 4, 4, 2]), np.array([3, 1]), cells, pbcs)
    counts = np.arange(20, dtype=np.int64)
    msd = np.arange(9.0).reshape(3, 3)
    res = attach_observables([{}, {}], plan, dict(n_samples=2, counts=counts, msd_sum=msd, vacf_sum=-msd), dt=0.5)
    o = res[0]['observables']
    assert o['every'] == 2 and o['n_samples'] == 2 and o['kinds'].tolist() == [1, 4] and res[1]['observables']['kinds'].tolist() == [2]
    assert np.array_equal(o['rdf']['counts'], counts[:16].reshape(2, 2, 4)) and o['rdf']['edges'].tolist() == [0, 0.5, 1.0, 1.5, 2.0]
    shell = 4 / 3 * np.pi * (np.array([0.5, 1.0, 1.5, 2.0]) ** 3 - np.array([0, 0.5, 1.0, 1.5]) ** 3)
    assert np.allclose(o['rdf']['g'][0, 1], counts[4:8] / (2 * 1 * (2 / 125.0) * shell), rtol=1e-14)
    assert res[1]['observables']['rdf']['g'] is None and np.array_equal(res[1]['observables']['rdf']['counts'][0, 0], counts[16:])
    assert o['lag_times'].tolist() == [0.0, 1.0, 2.0] and o['n_origins'].tolist() == [1, 1, 0]
    assert np.allclose(o['msd'][1, :2], msd[1, :2] / 2) and np.isnan(o['msd'][:, 2]).all()
    assert np.allclose(o['msd_all'][:2], (msd[0, :2] + msd[1, :2]) / 3) and np.allclose(o['vacf'][0, :2], -msd[0, :2])


# ------------------------------------------------------------------------------------------------ the binding
def test_entry_points_are_declared_bound_and_built():
    from sevennet_amd import _lib, build
    assert 'snet_observe.hip' in build.STATIC_SOURCES and _lib.ABI_VERSION == 4
    with open(os.path.join(ROOT, 'include', 'snet_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert int(re.search(r'#define SNET_ABI_VERSION (\d+)', text).group(1)) == 4
    for name, n_args in (('snet_obs_rdf', 16), ('snet_obs_correlate', 20)):
        decl = re.search(r'\bint ' + name + r'\s*\(([^)]*)\)', text).group(1)
        assert len(decl.split(',')) == n_args == len(_lib.SIGNATURES[name][1]), name
        assert decl.split(',')[-1].strip() == 'void *stream'
    with open(os.path.join(ROOT, 'sevennet_amd', 'csrc', 'snet_observe.hip')) as f:
        src = f.read()
    assert '#include "snet_system.h"' in src and src.count('#pragma clang fp contract(off)') >= 3
    for helper in ('segment(', 'block_sum<', 'det3(', 'inv3(', 'row_mul('):
        assert helper in src, helper
    assert 'atomicAdd' in src and 'double' not in ''.join(l for l in src.splitlines() if 'atomicAdd' in l)   # integer atomics only
