"""GPU: batched nudged elastic band -- the force kernel against its fp64 restatement (neb_ref), the band loop on a potential
whose saddle point is known in closed form, and the driver and the public surfaces on a model: two rattled vacancy hops in the
2 x 1 x 1 diamond cell (15 atoms, three moving images each) and a five-atom molecule without a cell (one moving image)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import neb_ref
from helpers import oracle_model
from test_batch_gpu import Z, _calc, _systems
from test_relax_gpu import D3_CUT, DEV, _Atoms, _oracle

pytestmark = pytest.mark.gpu

TRICLINIC = np.array([[9.0, 0.0, 0.0], [1.5, 8.0, 0.0], [0.7, -1.1, 10.0]])


# ------------------------------------------------------------------------------------------------ the kernel
def _synthetic_band(rng, n, m, cell, pbc, energies=None, fixed=None, straddle=False, k=0.1, still=False):
    """one band for the kernel tests: a noisy line of m + 2 images, fp32 forces plus fp64 extra forces, energies split in two"""
    a = rng.uniform(0.0, 4.0, (n, 3))
    step = rng.normal(0.0, 0.15, (n, 3))
    images = a[None] + np.arange(m + 2)[:, None, None] * step[None] + rng.normal(0.0, 0.03, (m + 2, n, 3))
    if still:
        images[:] = a[None]
    if straddle:   # every second atom of the later images sits one cell further along the first lattice vector
        images[2:, ::2] += np.asarray(cell)[0]
    if energies is None:   # distinct by at least 1e-3
        energies = rng.permutation(m + 2) * 0.37 + rng.uniform(0.0, 0.36, m + 2)
        assert np.diff(np.sort(energies)).min() >= 1e-3
    energies = np.asarray(energies, np.float64)
    e_extra = rng.normal(0.0, 0.5, m + 2)
    return dict(images=images, E=energies, e_model=energies - e_extra, e_extra=e_extra, f32=rng.normal(0.0, 1.0, (m, n, 3)).astype(np.float32),
                fx=rng.normal(0.0, 1e-2, (m, n, 3)), cell=np.asarray(cell, np.float64), pbc=list(pbc), k=k,
                fixed=None if fixed is None else np.asarray(fixed, bool))


def _four_bands(pattern):
    rng = np.random.default_rng(21)
    open_ = (np.zeros((3, 3)), [False] * 3)
    energies = {'a': [0.0, 1.0, 2.0, 1.5, 3.0],    # rising, maximum with Ep > Em, minimum with Ep > Em
                'b': [3.0, 2.0, 2.5, 1.0, 0.0],    # minimum with Ep < Em, maximum with Ep < Em, falling
                'c': [1.0, 2.0, 1.0, 0.5, 0.2]}[pattern]   # the exact tie Ep == Em, falling, falling
    return [_synthetic_band(rng, 1, 1, *open_, still=pattern == 'c'),                       # smallest case (pattern c: zero tangent)
            _synthetic_band(rng, 5, 3, *open_, energies=energies, k=0.3),                  # the tangent branches
            _synthetic_band(rng, 300, 6, np.diag([30.0, 31.0, 32.0]), [True] * 3, k=0.05),   # more atoms than threads
            _synthetic_band(rng, 64, 2, TRICLINIC, [True, True, True], fixed=rng.random(64) < 0.25, straddle=True)]


BRANCHES = {'a': ['rising', 'maximum_up', 'minimum_up'], 'b': ['minimum_down', 'maximum_down', 'falling'],
            'c': ['maximum_tie', 'falling', 'falling']}


def _launch(bands, climb, active=None, nan_at=None, seg_ptr=None, end_ptr=None):
    """one snet_neb_forces launch over `bands` -> (f_neb per band [m,n,3], imax, active, status); nan_at = (band, interior image)
    replaces that image's energy by a NaN; seg_ptr / end_ptr replace the offsets that follow from the bands"""
    from sevennet_amd import neb
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)   # noqa: E731
    f64, i32 = torch.float64, torch.int32
    B = len(bands)
    m = [b['images'].shape[0] - 2 for b in bands]
    n = [b['images'].shape[1] for b in bands]
    e_model = [b['e_model'].copy() for b in bands]
    if nan_at is not None:
        e_model[nan_at[0]][1 + nan_at[1]] = np.nan
    padded, inv = neb.mic_cells(np.stack([b['cell'] for b in bands]), np.array([b['pbc'] for b in bands]))
    fixed = np.concatenate([np.tile(np.zeros(nb, bool) if b['fixed'] is None else b['fixed'], mb) for b, mb, nb in zip(bands, m, n)])
    N = sum(mb * nb for mb, nb in zip(m, n))
    f_neb = torch.full((N, 3), 123.0, dtype=f64, device=DEV)
    imax = torch.full((B,), -7, dtype=i32, device=DEV)
    act = t(np.ones(B) if active is None else active, i32)
    status = torch.zeros(B, dtype=i32, device=DEV)
    e_end = np.array([[b['e_model'][0] + b['e_extra'][0], b['e_model'][-1] + b['e_extra'][-1]] for b in bands])
    neb.neb_forces(t(np.concatenate([b['images'][1:-1].reshape(-1, 3) for b in bands]), f64),
                   t(np.concatenate([b['f32'].reshape(-1, 3) for b in bands]), torch.float32),
                   t(np.concatenate([e[1:-1] for e in e_model]), f64),
                   t(np.concatenate([[0], np.cumsum(np.repeat(n, m))]) if seg_ptr is None else seg_ptr, i32),
                   t(np.concatenate([[0], np.cumsum(m)]), i32),
                   t(np.concatenate([b['images'][[0, -1]].reshape(-1, 3) for b in bands]), f64),
                   t(np.concatenate([[0], np.cumsum(2 * np.array(n))]) if end_ptr is None else end_ptr, i32), t(e_end, f64),
                   t(padded.reshape(B, 9), f64),
                   t(inv.reshape(B, 9), f64), t(np.array([b['pbc'] for b in bands]), i32), t([b['k'] for b in bands], f64), act, status,
                   f_neb, imax, climb=climb, forces_extra=t(np.concatenate([b['fx'].reshape(-1, 3) for b in bands]), f64),
                   energy_extra=t(np.concatenate([b['e_extra'][1:-1] for b in bands]), f64), fixed=t(fixed, i32))
    torch.cuda.synchronize()
    flat = f_neb.cpu().numpy()
    ptr = np.concatenate([[0], np.cumsum([mb * nb for mb, nb in zip(m, n)])])
    return ([flat[ptr[b]:ptr[b + 1]].reshape(m[b], n[b], 3) for b in range(B)], imax.cpu().numpy(), act.cpu().numpy(),
            status.cpu().numpy())


def _restated(band, climb):
    """neb_ref on the bits the kernel sees: fp32 forces widened plus the fp64 ones, the two energy parts added in fp64, and the
    inverse cell the driver computes"""
    from sevennet_amd import neb
    padded, inv = neb.mic_cells(band['cell'][None], np.array([band['pbc']]))
    return neb_ref.neb_forces(band['images'], band['f32'].astype(np.float64) + band['fx'], band['e_model'] + band['e_extra'], padded[0],
                              band['pbc'], band['k'], climb, band['fixed'], inv=inv[0])


@pytest.mark.parametrize('climb', [False, True])
@pytest.mark.parametrize('pattern', ['a', 'b', 'c'])
def test_kernel_equals_the_restatement(pattern, climb):
    """imax exactly; f_neb within 1e-11 of the band's largest |component|: fp64 sums of at most 900 terms in another order
    (900 x 1.1e-16 ~ 1e-13, times the few operations that follow, times 10: the reasoning of test_relax_gpu._compare)"""
    bands = _four_bands(pattern)
    got, imax, active, status = _launch(bands, climb)
    assert active.tolist() == [1] * 4 and status.tolist() == [0] * 4
    for b, band in enumerate(bands):
        want, top, info = _restated(band, climb)
        assert imax[b] == top, (b, imax[b], top)
        err, scale = np.abs(got[b] - want).max(), np.abs(want).max()
        print(f'pattern {pattern}, climb {climb}, band {b}: max error {err:.2e} at scale {scale:.2e}, branches {[w["branch"] for w in info]}')
        assert err <= 1e-11 * scale, (b, err, scale)
        if band['fixed'] is not None:
            assert band['fixed'].any() and np.array_equal(got[b][:, band['fixed']], np.zeros_like(got[b][:, band['fixed']]))
        if b == 1:
            assert [w['branch'] for w in info] == BRANCHES[pattern]
        if b == 0 and pattern == 'c':
            assert info[0]['branch'] == 'zero'
        if b == 3:   # the straddling pair went the short way (32 atoms a whole lattice vector of 9 A away would make it 51 A long)
            assert info[0]['tp'] < 3.0 and info[1]['tm'] < 3.0
    if climb:   # the climbing branch changed something in every band
        plain, _, _, _ = _launch(bands, False)
        assert all(not np.array_equal(p, g) for p, g in zip(plain[1:], got[1:]))


def test_inactive_bands_are_skipped_and_a_nan_energy_switches_its_band_off():
    bands = _four_bands('a')
    ref, imax0, _, _ = _launch(bands, True)
    got, imax, active, status = _launch(bands, True, active=[1, 0, 1, 1])
    assert np.array_equal(got[1], np.zeros_like(got[1]))                       # zero rows, written over the 123.0 they held
    assert imax[1] == -7 and active.tolist() == [1, 0, 1, 1] and status.tolist() == [0] * 4   # nothing else of it touched
    for b in (0, 2, 3):
        assert np.array_equal(got[b], ref[b]) and imax[b] == imax0[b]
    got, imax, active, status = _launch(bands, True, nan_at=(2, 3))            # a NaN energy as input: nothing is provoked
    assert status.tolist() == [0, 0, 2, 0] and active.tolist() == [1, 1, 0, 1]
    for w in (2, 3, 4):   # the image itself and both neighbours read the NaN: their rows are zero
        assert np.array_equal(got[2][w], np.zeros_like(got[2][w]))
    assert np.isfinite(got[2]).all()
    for b in (0, 1, 3):
        assert np.array_equal(got[b], ref[b]) and imax[b] == imax0[b]


def test_a_band_whose_offsets_do_not_fit_is_refused_before_a_neighbour_is_read():
    """images of unequal size within a band, and endpoint rows that are not two images long: status 3, active 0 and zero rows for
    that band (every offset stays inside the arrays: the kernel compares sizes, it reads no neighbour of such a band), the other
    bands as without it"""
    bands = _four_bands('a')
    ref, imax0, _, _ = _launch(bands, False)
    # band 1 (5 atoms, 3 moving images = rows 1 .. 16): the boundary between its first two images moved by one row
    seg = np.concatenate([[0], np.cumsum(np.repeat([1, 5, 300, 64], [1, 3, 6, 2]))])
    seg[2] += 1
    got, imax, active, status = _launch(bands, False, seg_ptr=seg)
    assert status.tolist() == [0, 3, 0, 0] and active.tolist() == [1, 0, 1, 1] and imax[1] == -7
    assert np.array_equal(got[1], np.zeros_like(got[1]))
    for b in (0, 2, 3):
        assert np.array_equal(got[b], ref[b]) and imax[b] == imax0[b]
    # band 3's endpoint rows one row short of two images (its end_ptr range is 127 rows, not 128)
    end = np.concatenate([[0], np.cumsum(2 * np.array([1, 5, 300, 64]))])
    end[4] -= 1
    got, imax, active, status = _launch(bands, False, end_ptr=end)
    assert status.tolist() == [0, 0, 0, 3] and active.tolist() == [1, 1, 1, 0]
    assert np.array_equal(got[3], np.zeros_like(got[3]))
    for b in (0, 1, 2):
        assert np.array_equal(got[b], ref[b])


# ------------------------------------------------------------------------------------------------ the loop, analytic potential
class _SaddleForces:
    """neb_ref.saddle_potential in torch on the device, behind the call interface of batch.BatchForces: the fp32 forces are
    zero, the fp64 forces go through the extra slot, the energies are per image (summed over the atoms in index order)"""

    def __init__(self, n_atoms_per_image):
        self.n_atoms = np.asarray(n_atoms_per_image, np.int64)
        self.engine = SimpleNamespace(dev=torch.device(DEV))
        self.n_force_calls = self.system_steps_evaluated = 0

    def __call__(self, pos, ids=None, **kw):
        ids = np.arange(len(self.n_atoms)) if ids is None else np.asarray(ids, np.int64)
        n = self.n_atoms[ids]
        seg = np.concatenate([[0], np.cumsum(n)])
        a = neb_ref.SADDLE_A
        x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
        u = y - a * (1.0 - x * x)
        e_atom = (x * x - 1.0) ** 2 + 2.0 * u * u + 2.0 * z * z
        f = -torch.stack([4.0 * x * (x * x - 1.0) + 4.0 * u * (2.0 * a * x), 4.0 * u, 4.0 * z], dim=1)
        energy = torch.empty(len(ids), dtype=torch.float64, device=pos.device)
        j = 0
        while j < len(ids):   # runs of images with the same atom count: their energies by explicit adds in atom order
            j1 = j
            while j1 < len(ids) and n[j1] == n[j]:
                j1 += 1
            block = e_atom[int(seg[j]):int(seg[j1])].reshape(j1 - j, int(n[j]))
            acc = block[:, 0].clone()
            for c in range(1, int(n[j])):
                acc = acc + block[:, c]
            energy[j:j1] = acc
            j = j1
        self.n_force_calls += 1
        self.system_steps_evaluated += len(ids)
        g = SimpleNamespace(seg_ptr=torch.as_tensor(seg.astype(np.int32)).to(pos.device), seg_ptr_host=seg)
        out = dict(forces=torch.zeros(len(pos), 3, dtype=torch.float32, device=pos.device), energy_per_system=energy)
        return g, out, f.contiguous(), torch.zeros(len(ids), dtype=torch.float64, device=pos.device)


SADDLE_BANDS = [(3, 5), (3, 4), (7, 3)]
SADDLE_FMAX = 1e-3


def _saddle_loop(which):
    from sevennet_amd.neb import neb_loop
    from sevennet_amd.relax import check_fire_params
    bands = [neb_ref.saddle_band(n, m) for n, m in which]
    M = [b.shape[0] for b in bands]
    forces = _SaddleForces(np.repeat([b.shape[1] for b in bands], M))
    B = len(bands)
    final, n_steps, status, info = neb_loop(
        forces, M, np.concatenate([b.reshape(-1, 3) for b in bands]), np.zeros((B, 3, 3)), np.zeros((B, 3), bool), fmax=SADDLE_FMAX,
        steps=400, repack_below=1.0, params=check_fire_params(SADDLE_FMAX, 400, 1.0, {}), k=np.full(B, 0.1), climb=True)
    flat = final.cpu().numpy()
    ptr = np.concatenate([[0], np.cumsum([b.size // 3 for b in bands])])
    return [flat[ptr[b]:ptr[b + 1]].reshape(bands[b].shape) for b in range(B)], n_steps, status, info


def test_loop_finds_the_known_saddle_with_the_restatements_step_counts():
    images, n_steps, status, info = _saddle_loop(SADDLE_BANDS)
    cos = []
    for b, (n, m) in enumerate(SADDLE_BANDS):
        ref = neb_ref.neb_relax(neb_ref.saddle_band(n, m), neb_ref.saddle_potential, np.zeros((3, 3)), [False] * 3, fmax=SADDLE_FMAX,
                                steps=400, k=0.1, climb=True)
        cos += [abs(w['cos']) for w in ref['log'][1:] if w['cos'] is not None]
        energies = np.array([neb_ref.saddle_potential(p)[0] for p in images[b]])
        barrier = energies.max() - energies[0]
        print(f'band {b} (n, m) = ({n}, {m}): {n_steps[b]} steps (restatement {ref["n_steps"]}), |barrier - 1| = {abs(barrier - 1):.2e}')
        assert status[b] == 1 and ref['converged']
        assert abs(barrier - 1.0) <= n * SADDLE_FMAX ** 2 / 4            # the bound of test_neb_cpu
        assert n_steps[b] == ref['n_steps']
        assert np.array_equal(images[b][[0, -1]], neb_ref.saddle_band(n, m)[[0, -1]])
    print(f'closest |cos(F, v)| to a tie over all steps of the restatement: {min(cos):.3e}')
    assert info['n_repacks'] >= 1
    assert info['fire_launches'] == max(n_steps) + 1 and info['n_force_calls'] == info['fire_launches'] + 1   # + the endpoints
    alone, steps_alone, _, _ = _saddle_loop(SADDLE_BANDS[1:2])
    assert steps_alone[0] == n_steps[1] and np.array_equal(alone[0], images[1])   # bit for bit, in the batch or alone


# ------------------------------------------------------------------------------------------------ the driver on a model
K_MODEL = 0.1


def model_bands():
    """[(types [n], images [M,n,3], cell, pbc)]: two vacancy hops in the rattled 2 x 1 x 1 diamond cell (site 4 is removed, its
    neighbour, site 0, moves into the hole: 2.35 A, below half the smallest cell height of 2.7 A) with three moving images,
    and the molecule of the batch tests with one atom displaced and one moving image"""
    from sevennet_amd.neb import interpolate_band
    from sevennet_amd.neighbor import diamond_cubic
    out = []
    for seed in (0, 1):
        pos, cell = diamond_cubic(5.431, (2, 1, 1), 0.05, seed)
        keep = np.arange(len(pos)) != 4
        initial, final = pos[keep].copy(), pos[keep].copy()
        final[0] = pos[4]
        types = np.random.default_rng(seed).integers(0, 2, len(pos))[keep]
        out.append((types, interpolate_band(initial, final, 5, cell, [True] * 3), cell, [True] * 3))
    types, mol, cell, pbc = _systems(2)[4]
    moved = mol.copy()
    moved[4] += [0.3, -0.4, 0.5]
    out.append((types, interpolate_band(mol, moved, 3), cell, pbc))
    return out


def _neb_args(bands):
    return ([np.array(Z)[b[0]] for b in bands], [b[1] for b in bands], np.stack([b[2] for b in bands]), np.array([b[3] for b in bands]))


@pytest.fixture(scope='module')
def model():
    from sevennet_amd.shapes import mini_sevennet_0_config
    calc, cfg, sd = _calc(mini_sevennet_0_config())
    return SimpleNamespace(calc=calc, cfg=cfg, sd=sd, orc=oracle_model(cfg, sd))


FIRST_STEPS = 5
# reference against reference on the CPU (neb_ref driven by the fp32 oracle against neb_ref driven by the fp64 oracle, the bands
# of model_bands(), FIRST_STEPS steps): the largest position deviation, per band
REF32_VS_REF64 = (1.5e-9, 2.2e-9, 5.7e-10)


def test_first_steps_follow_the_oracle_trajectory(model):
    """positions after 5 steps against the restatement driven by the fp64 oracle's energies and forces.  The starting bound is
    that of test_relax_gpu.test_first_steps_follow_the_oracle_trajectory, 1e-4 (sum_k dt_k)^2 A = 6.25e-6 A here (the first step
    halves dt: five moves of 0.05); the energy-weighted tangent of an extremum image turns an energy error into a tangent
    error, for which three times the deviation of the restatement driven by the fp32 oracle from the one driven by the fp64
    oracle over the same steps is allowed on top (REF32_VS_REF64: at most 2.2e-9 A, so 6.6e-9 A, measured on the CPU, reference
    against reference).  Needs the same decisions on both sides: the smallest energy difference a tangent branch rests on
    (1.4e-4 / 3.1e-3 / 8.3e-5 eV for the three bands when this was written) is more than ten times the engine's energy
    tolerance of 1e-6 |E| + 1e-6 eV (3.3e-6 / 4.3e-6 / 1.9e-6 eV), and the cosine of F and v is above 0.5 from the second step
    on (1.0000 when this was written)."""
    bands = model_bands()
    res = model.calc.neb_many(*_neb_args(bands), fmax=1e-4, steps=FIRST_STEPS, k=K_MODEL)
    for b, (types, images, cell, pbc) in enumerate(bands):
        ref = neb_ref.neb_relax(images, lambda p: _oracle(model, types, p, cell, pbc), cell, pbc, fmax=1e-4, steps=FIRST_STEPS, k=K_MODEL)
        assert ref['n_steps'] == FIRST_STEPS and res[b]['n_steps'] == FIRST_STEPS and res[b]['status'] == 'steps'
        margin = min(w['margin'] for step in ref['log'] for w in step['images'])
        e_err = 1e-6 * np.abs(ref['energies']).max() + 1e-6     # the engine's energy tolerance (test_relax_gpu._check_relaxed)
        cos = min(w['cos'] for w in ref['log'][1:])
        got = np.stack([im['positions'] for im in res[b]['images']])
        err = np.abs(got - ref['images']).max()
        tol = 1e-4 * sum(ref['dts']) ** 2 + 3.0 * REF32_VS_REF64[b]
        print(f'band {b}: max |dr| {err:.3e} A (bound {tol:.3e}), smallest tangent margin {margin:.3e} eV (energy error {e_err:.1e}), '
              f'min cos {cos:.4f}')
        assert margin > 10 * e_err and cos > 0.5
        assert err <= tol, (b, err, tol)


@pytest.fixture(scope='module')
def relaxed(model):
    bands = model_bands()
    res = model.calc.neb_many(*_neb_args(bands), fmax=1e-4, steps=30, k=K_MODEL, climb=True)
    return bands, res, dict(model.calc.neb_info)


def test_results_are_compute_at_the_returned_positions(model, relaxed):
    bands, res, info = relaxed
    assert info['fire_launches'] == 30 and info['n_force_calls'] == 32   # the endpoints before, all images after
    one = model.calc.compute(np.array(Z)[bands[0][0]], bands[0][1][0], bands[0][2], bands[0][3])
    for b, (types, images, cell, pbc) in enumerate(bands):
        r = res[b]
        assert set(r) == {'images', 'converged', 'n_steps', 'status', 'neb_fmax', 'imax', 'barrier', 'barrier_reverse'}
        assert r['n_steps'] == 30 and r['status'] == 'steps' and r['converged'] is False and len(r['images']) == len(images)
        assert np.array_equal(r['images'][0]['positions'], images[0]) and np.array_equal(r['images'][-1]['positions'], images[-1])
        assert not np.array_equal(r['images'][1]['positions'], images[1])
        for im in r['images']:   # the tolerances of test_relax_gpu._check_relaxed
            assert set(im) == set(one) | {'positions'}
            single = model.calc.compute(np.array(Z)[types], im['positions'], cell, pbc)
            assert abs(im['energy'] - single['energy']) <= 1e-6 * abs(single['energy']) + 1e-6
            assert np.abs(im['forces'] - single['forces']).max() <= 2e-5 * max(1.0, np.abs(single['forces']).max())
        pos = np.stack([im['positions'] for im in r['images']])
        energies = np.array([im['energy'] for im in r['images']])
        f_neb, top, _ = neb_ref.neb_forces(pos, np.stack([im['forces'] for im in r['images']]), energies, cell, pbc, K_MODEL, climb=True)
        fm = np.sqrt((f_neb ** 2).sum(-1).max())
        print(f'band {b}: neb_fmax {r["neb_fmax"]:.6f} eV/A, imax {r["imax"]}, barrier {r["barrier"]:.6f} / {r["barrier_reverse"]:.6f} eV')
        assert r['imax'] == top + 1 and abs(r['neb_fmax'] - fm) <= 1e-10 * fm
        assert r['barrier'] == energies.max() - energies[0] and r['barrier_reverse'] == energies.max() - energies[-1]


def test_two_runs_are_identical(model, relaxed):
    bands, res, _ = relaxed
    again = model.calc.neb_many(*_neb_args(bands), fmax=1e-4, steps=30, k=K_MODEL, climb=True)
    for x, y in zip(res, again):
        assert all(x[key] == y[key] for key in ('n_steps', 'status', 'neb_fmax', 'imax', 'barrier', 'barrier_reverse'))
        for p, q in zip(x['images'], y['images']):
            assert np.array_equal(p['positions'], q['positions']) and p['energy'] == q['energy'] and np.array_equal(p['forces'], q['forces'])


def test_no_steps_and_the_atoms_surface(model, relaxed):
    bands, res, _ = relaxed
    none = model.calc.neb_many(*_neb_args(bands), fmax=1e-4, steps=0, k=K_MODEL)
    assert model.calc.neb_info['fire_launches'] == 0
    for r, band in zip(none, bands):
        assert r['n_steps'] == 0 and r['status'] == 'steps'
        assert np.array_equal(np.stack([im['positions'] for im in r['images']]), band[1])
    atoms = [[_Atoms(np.array(Z)[t], p, cell, pbc) for p in images] for t, images, cell, pbc in bands]
    got = model.calc.neb_many_atoms(atoms, fmax=1e-4, steps=30, k=K_MODEL, climb=True)
    for band_atoms, r, q, band in zip(atoms, got, res, bands):
        for j, (a, im, ref_im) in enumerate(zip(band_atoms, r['images'], q['images'])):
            assert np.array_equal(a.get_positions(), im['positions']) and np.array_equal(im['positions'], ref_im['positions'])
        assert np.array_equal(band_atoms[0].get_positions(), band[1][0]) and np.array_equal(band_atoms[-1].get_positions(), band[1][-1])
        assert not np.array_equal(band_atoms[1].get_positions(), band[1][1])
    with pytest.raises(ValueError, match='returned forces without energies'):
        model.calc.neb_many(*_neb_args(bands), steps=2, extra=lambda pos, seg_ptr, ids: torch.zeros_like(pos))
    with pytest.raises(ValueError, match='Model do not know atomic number: 79'):
        model.calc.neb_many([[79]], [np.zeros((3, 1, 3))], np.zeros((1, 3, 3)), [False] * 3)


def test_d3_sum_runs_on_the_host_term_and_on_the_device_term(model):
    """the device term's forces and energies are the host term's bit for bit at fixed cells (test_d3_device_gpu), so the bands are"""
    from sevennet_amd.d3 import SevenNetD3Calculator
    calc = SevenNetD3Calculator((model.cfg, model.sd), file_type='model_instance', device=DEV, **D3_CUT)
    bands = model_bands()
    host = calc.neb_many(*_neb_args(bands), fmax=1e-4, steps=5, k=K_MODEL, d3_term='host')
    info = dict(calc.neb_info)
    dev = calc.neb_many(*_neb_args(bands), fmax=1e-4, steps=5, k=K_MODEL, d3_term='device')
    plain = model.calc.neb_many(*_neb_args(bands), fmax=1e-4, steps=5, k=K_MODEL)
    assert calc.neb_info == info and info['fire_launches'] == 5
    for h, d, p in zip(host, dev, plain):
        assert h['n_steps'] == d['n_steps'] == 5
        for key in ('neb_fmax', 'barrier', 'barrier_reverse'):
            assert np.isfinite(h[key]) and h[key] == d[key]
        assert h['imax'] == d['imax']
        for x, y, z in zip(h['images'], d['images'], p['images']):
            assert np.isfinite(x['positions']).all() and np.isfinite(x['forces']).all() and np.isfinite(x['energy'])
            assert np.array_equal(x['positions'], y['positions']) and x['energy'] == y['energy'] and np.array_equal(x['forces'], y['forces'])
            assert x['energy'] != z['energy']   # the D3 share is in
        assert not np.array_equal(h['images'][1]['positions'], p['images'][1]['positions'])
