"""GPU: atoms and Cartesian components held fixed -- the four masked step kernels against their fp64 restatement (fixed_ref) and
against the unmasked kernels bit for bit, and `fixed_list` in relax_many / md_many on a model: the three rattled two-species
diamond cells of test_relax_gpu, half of cell 0's atoms held, the z components of cell 1, three atoms of cell 2.

Kernel tests use systems of 1, 5, 64 and 300 atoms in one launch (300: a second trip of the 256-thread loop and a partial wave)
with everything held, nothing held, whole atoms held and random component bits.

Random weights have no repulsion, so the step cap of the model test was fixed on the CPU first (MODEL_STEPS)."""
import numpy as np
import pytest
import torch

import cellrelax_ref
import fixed_ref
import md_ref
import relax_ref
from test_cell_relax_gpu import C0, F_INIT
from test_cell_relax_gpu import _DeviceState as _CellState
from test_cell_relax_gpu import _compare as _compare_cell
from test_md_batch_gpu import DT, MASS_OF, _md_args, _position_bound, _start_velocities
from test_md_batch_gpu import _DeviceState as _MdState
from test_relax_gpu import D3_CUT, DEV, FMAX, _all_systems, _args, _cells, _oracle, model  # noqa: F401  (model: the fixture)
from test_relax_gpu import _DeviceState as _FireState
from test_relax_gpu import _compare as _compare_fire

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 64, 300]
STIFFNESS = [40.0, 3.0, 0.6, 5.0]
# with the fp64 oracle driving fixed_ref.fire_relax on the CPU at fmax 0.02 the masked cells of _masks() converge after 31 / 20 / 41
# force evaluations (the free ones after 46 / 25 / 29, test_relax_gpu), the oracle's largest force over the free components then
# being 0.0132 / 0.0184 / 0.0179 eV/A; the cap is twice the largest count
ORACLE_EVALS = (31, 20, 41)
MODEL_STEPS = 2 * max(ORACLE_EVALS)


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _h(t):
    return t.cpu().numpy()


def _kernel_masks(rng, sizes=SIZES):
    """everything held (the one atom), nothing held, whole atoms held (half of them), random component bits"""
    masks = [np.full(sizes[0], 7), np.zeros(sizes[1], int), np.where(rng.random(sizes[2]) < 0.5, 7, 0), rng.integers(0, 8, sizes[3])]
    assert masks[2].any() and not masks[2].all() and set(masks[3].tolist()) == set(range(8))
    return masks


def _poison(forces, held):
    """NaN where a component is held: what the masked kernels must never look at"""
    return np.where(held, np.nan, forces).astype(forces.dtype)


# ------------------------------------------------------------------------------------------------ snet_fire_step_fixed
def _fire_launch(states, forces32, fmax, hold=None, extra=None):
    from sevennet_amd.relax import check_fire_params, fire_step
    dev = _FireState(states)
    x = None if extra is None else _t(extra, torch.float64)
    fire_step(dev.pos, dev.vel, _t(forces32, torch.float32), dev.seg_ptr, dev.dt, dev.alpha, dev.n_pos, dev.active, dev.n_steps,
              dev.fmax_sys, dev.n_active, fmax, check_fire_params(fmax, 1, 0.5, {}), x, None if hold is None else _t(hold, torch.int32))
    torch.cuda.synchronize()
    return dev


def _same_bits(a, b, names):
    for name in names:
        x, y = _h(getattr(a, name)), _h(getattr(b, name))
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == 'f'), name


FIRE_OUTPUTS = ('pos', 'vel', 'dt', 'alpha', 'n_pos', 'active', 'n_steps', 'fmax_sys', 'n_active')


def test_fire_kernel_follows_the_restatement_step_by_step():
    """40 steps of harmonic fp32 forces, the device state rebuilt from the restatement's each time: scalars exactly, pos / vel to
    the tolerance of test_relax_gpu._compare; held positions keep the bits they started with and held velocities are exactly 0
    after every step; the forces handed to the kernel are NaN on every held component"""
    rng = np.random.default_rng(11)
    masks = _kernel_masks(rng)
    hold, held = np.concatenate(masks), [fixed_ref.components(m) for m in masks]
    states = [relax_ref.fire_init(rng.normal(0, 0.5, (n, 3))) for n in SIZES]
    x0 = np.concatenate([s['pos'] for s in states])
    seen = {'uphill': 0, 'downhill': 0, 'clipped': 0, 'frozen': 0}
    for it in range(40):
        forces = [(-k * s['pos']).astype(np.float32) for k, s in zip(STIFFNESS, states)]   # fp32, the same bits to both sides
        dev = _fire_launch(states, np.concatenate([_poison(f, m) for f, m in zip(forces, held)]), 0.01, hold)
        nxt = [fixed_ref.fire_step(s, f, m, 0.01) for s, f, m in zip(states, forces, masks)]
        states, what = [n[0] for n in nxt], [n[1] for n in nxt]
        _compare_fire(dev, states, what, [np.where(m, 0.0, f.astype(np.float64)) for f, m in zip(forces, held)])
        all_held = np.concatenate(held)
        assert np.array_equal(_h(dev.pos)[all_held], x0[all_held]) and not _h(dev.vel)[all_held].any(), it
        if it == 0:   # nothing free: switched off by the first launch, no step counted
            assert _h(dev.active).tolist() == [0, 1, 1, 1] and _h(dev.n_steps).tolist() == [0, 1, 1, 1] and _h(dev.fmax_sys)[0] == 0.0
        for w in what:
            seen['frozen' if w['branch'] is None else w['branch']] += 1
            seen['clipped'] += bool(w['clipped'])
    # both branches beyond the first step (the three systems that move start uphill: v = 0), clipped moves and frozen systems
    assert seen['uphill'] > 3 and seen['downhill'] > 0 and seen['clipped'] > 0 and seen['frozen'] > 0, seen
    assert not np.array_equal(_h(dev.pos)[~all_held], x0[~all_held])


def _moving_fire_states(rng, sizes):
    states = [relax_ref.fire_init(rng.normal(0, 0.5, (n, 3))) for n in sizes]
    for s in states:
        s['vel'] = rng.normal(0, 0.1, s['pos'].shape)
        s['n_steps'], s['n_pos'], s['dt'], s['alpha'] = 4, 7, 0.07, 0.09
    return states


def test_fire_kernel_identities():
    rng = np.random.default_rng(5)
    states = _moving_fire_states(rng, SIZES)
    states[1]['vel'] *= -1.0
    f32 = np.concatenate([(-k * s['pos']).astype(np.float32) for k, s in zip(STIFFNESS, states)])
    f64 = 1e-3 * np.sin(3.0 * np.concatenate([s['pos'] for s in states]))
    N = sum(SIZES)
    # an all-zero mask: snet_fire_step's bits in every output, with and without the second force array
    for extra in (None, f64):
        _same_bits(_fire_launch(states, f32, 0.01, np.zeros(N, int), extra), _fire_launch(states, f32, 0.01, None, extra), FIRE_OUTPUTS)
    # a NaN force on a held component, in either array, changes no output bit relative to a finite one there
    masks = _kernel_masks(rng)
    masks[0][:] = 3   # (the one atom keeps a free component, so that its system moves)
    hold, held = np.concatenate(masks), fixed_ref.components(np.concatenate(masks))
    clean = _fire_launch(states, f32, 0.01, hold, f64)
    _same_bits(_fire_launch(states, _poison(f32, held), 0.01, hold, _poison(f64, held)), clean, FIRE_OUTPUTS)
    _same_bits(_fire_launch(states, _poison(f32, held), 0.01, hold, f64), clean, FIRE_OUTPUTS)
    assert _h(clean.active).tolist() == [1] * 4 and np.isfinite(_h(clean.pos)).all()
    # garbage in a held velocity on entry is stored back as 0 and does not enter |v| (nor anything else)
    dirty = [dict(s, vel=np.where(fixed_ref.components(m), g, s['vel'])) for s, m, g in zip(states, masks, (np.nan, 1e300, -np.inf, 7.0))]
    zeroed = [dict(s, vel=np.where(fixed_ref.components(m), 0.0, s['vel'])) for s, m in zip(states, masks)]
    a, b = _fire_launch(dirty, f32, 0.01, hold, f64), _fire_launch(zeroed, f32, 0.01, hold, f64)
    _same_bits(a, b, FIRE_OUTPUTS)
    _same_bits(a, clean, FIRE_OUTPUTS)
    assert not _h(a.vel)[held].any() and _h(a.vel)[~held].all()
    x_in = np.concatenate([s['pos'] for s in states])
    assert np.array_equal(_h(a.pos)[held], x_in[held]) and (_h(a.pos)[~held] != x_in[~held]).all()


def test_entry_points_refuse_a_missing_mask():
    import ctypes as C
    from sevennet_amd import _lib
    lib = _lib.load()
    dev = _FireState([relax_ref.fire_init(np.ones((4, 3)))])
    f = _t(np.ones((4, 3)), torch.float32)
    P = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.snet_fire_step_fixed(P(dev.pos), P(dev.vel), P(f), None, 4, P(dev.seg_ptr), 1, P(dev.dt), P(dev.alpha), P(dev.n_pos),
                                  P(dev.active), P(dev.n_steps), P(dev.fmax_sys), P(dev.n_active), 0.01, 0.1, 1.0, 5, 1.1, 0.5, 0.1, 0.99,
                                  0.2, None, st)
    assert rc == 2 and b'snet_fire_step_fixed: null argument' in lib.snet_last_error()
    m, kT, ids, si, ek = _t(np.ones(4), torch.float64), _t([0.02], torch.float64), _t([0], torch.int32), _t([0], torch.int32), _t([0.0], torch.float64)
    rc = lib.snet_mdb_step_fixed(P(dev.pos), P(dev.vel), P(f), None, P(m), 4, P(dev.seg_ptr), P(ids), 1, P(kT), P(si), P(ek), 1.0, 1.0, 0.0,
                                 0, 3, None, st)
    assert rc == 2 and b'snet_mdb_step_fixed: null argument' in lib.snet_last_error()
    assert lib.snet_mdb_init_velocities_fixed(P(dev.vel), P(m), 4, P(dev.seg_ptr), P(ids), 1, P(kT), 0, 1, None, st) == 2
    torch.cuda.synchronize()
    assert _h(dev.pos).tolist() == np.ones((4, 3)).tolist() and _h(si).tolist() == [0]
    from sevennet_amd.relax import check_fire_params, fire_step
    with pytest.raises(ValueError, match='fire_step'):   # the Python wrapper checks dtype and shape of the mask before the call
        fire_step(dev.pos, dev.vel, f, dev.seg_ptr, dev.dt, dev.alpha, dev.n_pos, dev.active, dev.n_steps, dev.fmax_sys, dev.n_active,
                  0.01, check_fire_params(0.01, 1, 0.5, {}), None, _t(np.zeros(3), torch.int32))


# ------------------------------------------------------------------------------------------------ snet_fire_cell_step_fixed
CELL_SIZES = [2, 9, 300]


def _cell_setup(rng):
    """harmonic crystals (cellrelax_ref.harmonic_crystal) of 2, 9 and 300 atoms in the deformed triclinic cell of
    test_cell_relax_gpu; held: one of the two atoms, all nine, and about half of the 300 under assorted nonzero words"""
    cell = C0 @ F_INIT.T
    x0 = [rng.random((n, 3)) for n in CELL_SIZES]
    states = [cellrelax_ref.cell_fire_init(x @ cell + rng.normal(0, 0.1, x.shape), cell, cell0=C0) for x in x0]
    masks = [np.array([7, 0]), np.full(9, 7), np.where(rng.random(300) < 0.5, rng.integers(1, 8, 300), 0)]
    assert set(masks[2].tolist()) == set(range(8))
    return x0, states, masks


def _crystal_inputs(states, x0):
    out = []
    for s, x in zip(states, x0):
        _, f, W = cellrelax_ref.harmonic_crystal(s['pos'], s['cell'], x, C0 @ C0.T)
        out.append((f.astype(np.float32), np.array(cellrelax_ref.virial6(W))))   # fp32 forces, the same bits to both sides
    return out


def _cell_launch(states, forces32, virial, fmax, hold=None):
    from sevennet_amd.relax import check_cell_params, check_fire_params, fire_cell_step
    dev = _CellState(states)
    fire_cell_step(dev.pos, dev.vel, dev.cell, dev.vel_cell, dev.cell0, _t(forces32, torch.float32), _t(virial, torch.float64),
                   dev.seg_ptr, dev.dt, dev.alpha, dev.n_pos, dev.active, dev.n_steps, dev.status, dev.fmax_sys, dev.n_active, fmax,
                   check_fire_params(fmax, 1, 0.5, {}), check_cell_params(**cellrelax_ref.CELL), 0.0, None, None,
                   None if hold is None else _t(hold, torch.int32))
    torch.cuda.synchronize()
    return dev


CELL_OUTPUTS = FIRE_OUTPUTS + ('cell', 'vel_cell', 'status')


def test_cell_kernel_follows_the_restatement_and_held_atoms_move_with_the_cell():
    """15 steps against fixed_ref.cell_fire_step at the tolerances of test_cell_relax_gpu._compare; a held atom keeps its
    fractional coordinates to 1e-12 while its cell moves, and its reference-frame velocity is exactly 0"""
    rng = np.random.default_rng(17)
    x0, states, masks = _cell_setup(rng)
    hold = np.concatenate(masks)
    held = np.concatenate(masks) != 0
    frac0 = np.concatenate([s['pos'] @ np.linalg.inv(s['cell']) for s in states])
    cell_start = states[0]['cell'].copy()
    for it in range(15):
        inputs = _crystal_inputs(states, x0)
        f32 = np.concatenate([i[0] for i in inputs])
        dev = _cell_launch(states, _poison(f32, np.repeat(held[:, None], 3, 1)), np.stack([i[1] for i in inputs]), 1e-4, hold)
        nxt = [fixed_ref.cell_fire_step(s, f, w, m, 1e-4) for s, (f, w), m in zip(states, inputs, masks)]
        states = [n[0] for n in nxt]
        _compare_cell(dev, states, [n[1] for n in nxt])
        assert all(n[1]['branch'] is not None and not n[1]['guard'] for n in nxt), it   # every system moves in every step
        cells = _h(dev.cell).reshape(-1, 3, 3)
        sp = np.concatenate([[0], np.cumsum(CELL_SIZES)])
        frac = np.concatenate([_h(dev.pos)[sp[b]:sp[b + 1]] @ np.linalg.inv(cells[b]) for b in range(3)])
        assert np.abs(frac - frac0)[held].max() <= 1e-12, (it, np.abs(frac - frac0)[held].max())
        assert not _h(dev.vel)[held].any()
    assert np.abs(frac - frac0)[~held].max() > 1e-3 and np.abs(cells[0] - cell_start).max() > 1e-3   # the free atoms and the cells moved
    assert np.abs(cells[1] - cell_start).max() > 1e-3   # ... the cell of the system whose atoms are all held too


def test_cell_kernel_with_an_all_zero_mask_is_the_unmasked_kernel():
    rng = np.random.default_rng(18)
    x0, states, _ = _cell_setup(rng)
    for s in states:
        s['vel'], s['vel_cell'] = rng.normal(0, 0.05, s['pos'].shape), rng.normal(0, 0.05, (3, 3))
        s['n_steps'], s['n_pos'], s['dt'], s['alpha'] = 4, 7, 0.07, 0.09
    inputs = _crystal_inputs(states, x0)
    f32, w = np.concatenate([i[0] for i in inputs]), np.stack([i[1] for i in inputs])
    a, b = _cell_launch(states, f32, w, 1e-4, np.zeros(sum(CELL_SIZES), int)), _cell_launch(states, f32, w, 1e-4)
    _same_bits(a, b, CELL_OUTPUTS)
    assert _h(a.n_steps).tolist() == [5] * 3 and _h(a.status).tolist() == [0] * 3


# ------------------------------------------------------------------------------------------------ snet_mdb_step_fixed
def _md_launch(states, masses, kT, forces32, dt, c1, c2, seed, phase, hold=None, extra=None):
    from sevennet_amd.md import md_step
    dev = _MdState(states, masses, kT)
    x = None if extra is None else _t(extra, torch.float64)
    md_step(dev.pos, dev.vel, _t(forces32, torch.float32), dev.mass, dev.seg_ptr, dev.sys_id, dev.kT, dev.step_index, dev.e_kin, dt, c1,
            c2, seed, phase, x, None if hold is None else _t(hold, torch.int32))
    torch.cuda.synchronize()
    return dev


@pytest.mark.parametrize('gamma_dt', [0.0, 0.05], ids=['nve', 'langevin'])
def test_md_kernel_moves_the_free_components_as_the_unmasked_kernel_does(gamma_dt):
    """phases 2, 3, 3, 1: per launch the masked kernel (forces NaN on every held component) and snet_mdb_step on the same state.
    Free components of pos and vel: the same bits.  Held positions keep their bits, held velocities are exactly 0, e_kin follows
    fixed_ref to 1e-12 relative, pos / vel follow it to the tolerance of test_md_batch_gpu (1e-11 of the largest component)."""
    rng = np.random.default_rng(13)
    dt, seed = 0.5, 77
    masks = _kernel_masks(rng)
    hold, held = np.concatenate(masks), fixed_ref.components(np.concatenate(masks))
    masses = [rng.choice([1.008, 15.999, 28.0855], n) for n in SIZES]
    kT = md_ref.KB * np.array([100.0, 300.0, 600.0, 1000.0])
    c1, c2 = md_ref.langevin_coefficients(gamma_dt / dt, dt)
    states = [md_ref.md_init(rng.normal(0, 0.5, (n, 3)), rng.normal(0, 0.01, (n, 3))) for n in SIZES]   # (held velocities not 0 yet)
    x0 = np.concatenate([s['pos'] for s in states])
    for it, phase in enumerate((2, 3, 3, 1)):
        f32 = [(-k * s['pos']).astype(np.float32) for k, s in zip(STIFFNESS, states)]
        f64 = [1e-3 * np.sin(3.0 * s['pos']) for s in states]
        v_in = np.concatenate([s['vel'] for s in states])
        masked = _md_launch(states, masses, kT, _poison(np.concatenate(f32), held), dt, c1, c2, seed, phase, hold, _poison(np.concatenate(f64), held))
        plain = _md_launch(states, masses, kT, np.concatenate(f32), dt, c1, c2, seed, phase, None, np.concatenate(f64))
        for name in ('pos', 'vel'):
            assert np.array_equal(_h(getattr(masked, name))[~held], _h(getattr(plain, name))[~held]), (it, name)
        assert np.array_equal(_h(masked.pos)[held], x0[held]) and not _h(masked.vel)[held].any(), it
        assert not np.array_equal(_h(plain.vel)[held], np.zeros(held.sum())) and _h(masked.step_index).tolist() == _h(plain.step_index).tolist()
        total = [a.astype(np.float64) + b for a, b in zip(f32, f64)]
        nxt = [fixed_ref.md_step(s, f, m, mass, t, dt, c1, c2, seed, b, phase)
               for b, (s, f, m, mass, t) in enumerate(zip(states, total, masks, masses, kT))]
        states, e_kin = [x[0] for x in nxt], np.array([x[1] for x in nxt])
        assert _h(masked.step_index).tolist() == [s['step'] for s in states]
        for name in ('pos', 'vel'):
            want = np.concatenate([s[name] for s in states])
            err, scale = np.abs(_h(getattr(masked, name)) - want).max(), np.abs(want).max()
            assert err <= 1e-11 * scale, (it, name, err, scale)
        assert (np.abs(_h(masked.e_kin) - e_kin) <= 1e-12 * e_kin).all() and e_kin[0] == 0.0, (it, _h(masked.e_kin), e_kin)
        assert (_h(masked.e_kin)[2:] < _h(plain.e_kin)[2:]).all() and _h(masked.e_kin)[1] == _h(plain.e_kin)[1]
        if phase & 2:
            assert not np.array_equal(_h(masked.pos)[~held], x0[~held]) and not np.array_equal(v_in[~held], _h(masked.vel)[~held])
    # phase 0 writes e_kin and nothing else, under a mask too: held velocities stay whatever they were
    dirty = [dict(s, vel=s['vel'] + 1.0) for s in states]
    dev = _md_launch(dirty, masses, kT, np.zeros((sum(SIZES), 3)), dt, c1, c2, seed, 0, hold)
    assert np.array_equal(_h(dev.vel), np.concatenate([s['vel'] for s in dirty])) and np.array_equal(_h(dev.pos), np.concatenate([s['pos'] for s in dirty]))
    want = np.array([md_ref.kinetic_energy(m, np.where(fixed_ref.components(k), 0.0, s['vel'])) for m, k, s in zip(masses, masks, dirty)])
    assert (np.abs(_h(dev.e_kin) - want) <= 1e-12 * want).all()


# ------------------------------------------------------------------------------------------------ snet_mdb_init_velocities_fixed
def test_init_velocities_under_a_mask():
    from sevennet_amd.md import init_velocities
    rng = np.random.default_rng(6)
    sizes = SIZES + [1, 3]
    masks = _kernel_masks(rng) + [np.zeros(1, int), np.array([0, 2, 0])]   # + a free atom, and three atoms with one component held
    hold = np.concatenate(masks)
    masses = [rng.choice([1.008, 15.999, 28.0855], n) for n in sizes]
    kT = md_ref.KB * np.array([100.0, 300.0, 600.0, 1000.0, 200.0, 400.0])
    sp = np.concatenate([[0], np.cumsum(sizes)])
    seg, ids, seed = _t(sp, torch.int32), [4, 0, 9, 2, 7, 1], (5 << 32) | 6
    m_d, kT_d, id_d, hold_d = _t(np.concatenate(masses), torch.float64), _t(kT, torch.float64), _t(ids, torch.int32), _t(hold, torch.int32)

    def draw(remove_com, mask):
        vel = torch.full((sum(sizes), 3), np.nan, dtype=torch.float64, device=DEV)
        init_velocities(vel, m_d, seg, id_d, kT_d, seed, remove_com, mask)
        torch.cuda.synchronize()
        return _h(vel)
    for remove_com in (True, False):
        got, base = draw(remove_com, hold_d), draw(remove_com, None)
        assert np.array_equal(got, draw(remove_com, hold_d)) and not np.isnan(got).any()
        assert np.array_equal(draw(remove_com, torch.zeros_like(hold_d)), base)   # nothing held anywhere: the unmasked draw's bits
        for k, (n, m, mask) in enumerate(zip(sizes, masses, masks)):
            v, held = got[sp[k]:sp[k + 1]], fixed_ref.components(mask)
            if not held.any():   # a system with nothing held, among systems with something held: the unmasked draw's bits
                assert np.array_equal(v, base[sp[k]:sp[k + 1]]), (remove_com, k)
                continue
            assert not v[held].any(), (remove_com, k)
            want = fixed_ref.init_velocities(m, mask, kT[k], seed, ids[k], remove_com)
            assert np.abs(v - want).max() <= 1e-11 * max(np.abs(want).max(), 1e-300), (remove_com, k)
            if remove_com:
                dof = 3 * n - held.sum()
                assert abs(md_ref.kinetic_energy(m, v) - 0.5 * dof * kT[k]) <= 1e-12 * 0.5 * dof * kT[k], (k, dof)
                assert v[~held].all() or dof == 0
            else:   # the raw draw on the free components, untouched
                assert np.array_equal(v[~held], base[sp[k]:sp[k + 1]][~held])
        assert not got[0].any()                                   # the one atom, all of it held: zeros, no 0/0
        assert not got[sp[4]].any() if remove_com else got[sp[4]].all()   # the free atom: at rest once its centre of mass rests


# ------------------------------------------------------------------------------------------------ relax_many on a model
def _masks(systems):
    """half of cell 0's atoms as a bool [n], the z components of cell 1 as a bool [n,3], an index list in cell 2; None beyond"""
    n0, n1 = len(systems[0][1]), len(systems[1][1])
    z = np.zeros((n1, 3), bool)
    z[:, 2] = True
    return [np.arange(n0) % 2 == 0, z, [0, 5, 10]] + [None] * (len(systems) - 3)


def _held(systems):
    from sevennet_amd.fixed import held_components, hold_masks
    n = [len(s[1]) for s in systems]
    comp = held_components(hold_masks(_masks(systems), n))
    sp = np.concatenate([[0], np.cumsum(n)])
    return [comp[sp[b]:sp[b + 1]] for b in range(len(n))]


def _same_dicts(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            nan_ok = isinstance(x[k], np.ndarray) and x[k].dtype.kind == 'f'   # (the stress of a system without a cell is NaN)
            assert np.array_equal(x[k], y[k], equal_nan=nan_ok), k


@pytest.fixture(scope='module')
def relaxed(model):   # noqa: F811
    systems = _all_systems()
    res = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=MODEL_STEPS, fixed_list=_masks(systems), repack_below=0.5)
    return systems, res, dict(model.calc.relax_info)


def test_relax_many_holds_what_it_is_told_to_hold(model, relaxed):   # noqa: F811
    """with the fp64 oracle driving fixed_ref on the CPU the masked cells converge after ORACLE_EVALS force evaluations; the
    molecule and the atom, unmasked, are below fmax where they start"""
    systems, res, info = relaxed
    initial = model.calc.compute_many(*_args(systems))
    held = _held(systems)
    for b, (types, pos, cell, pbc) in enumerate(systems):
        r = res[b]
        assert r['converged'], b
        assert np.array_equal(r['fixed'], held[b]) and r['fixed'].dtype == bool
        assert np.array_equal(r['positions'][held[b]], pos[held[b]])   # the caller's bits
        f_orc = _oracle(model, types, r['positions'], cell, pbc)[1]
        fm_free = np.sqrt((np.where(held[b], 0.0, f_orc) ** 2).sum(1).max())
        fm_all = np.sqrt((f_orc ** 2).sum(1).max())
        print(f'system {b}: n_steps {r["n_steps"]}, oracle max|F| free {fm_free:.5f} / all {fm_all:.5f} eV/A, '
              f'E {initial[b]["energy"]:.6f} -> {r["energy"]:.6f}')
        assert fm_free < FMAX + 1e-4, (b, fm_free)
        one = model.calc.compute(_args(systems)[0][b], r['positions'], cell, pbc)   # `forces` stay the true forces, held atoms too
        assert np.abs(r['forces'] - one['forces']).max() <= 2e-5 * max(1.0, np.abs(one['forces']).max()), b
        if r['n_steps'] > 0:
            assert r['energy'] < initial[b]['energy'], (b, r['energy'], initial[b]['energy'])
            assert (r['positions'][~held[b]] != pos[~held[b]]).any()
        else:
            assert np.array_equal(r['positions'], pos)
    assert [r['n_steps'] for r in res[3:]] == [0, 0] and all(5 < r['n_steps'] < MODEL_STEPS for r in res[:3])
    assert info['fire_launches'] == max(r['n_steps'] for r in res) + 1


def test_relax_many_repacking_changes_nothing_under_a_mask(model, relaxed):   # noqa: F811
    systems, res, info = relaxed
    res0 = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=MODEL_STEPS, fixed_list=_masks(systems), repack_below=0)
    assert info['n_repacks'] >= 1 and model.calc.relax_info['n_repacks'] == 0   # (the mask was regathered with pos and vel)
    _same_dicts(res, res0)


def test_masks_that_hold_nothing_are_no_masks(model):   # noqa: F811
    systems = _all_systems()
    ref = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=12)
    nothing = [np.zeros(len(systems[0][1]), bool), np.zeros((len(systems[1][1]), 3), bool), [], None, None]
    for fl in (None, nothing):
        res = model.calc.relax_many(*_args(systems), fmax=FMAX, steps=12, fixed_list=fl)
        _same_dicts(res, ref)
        assert 'fixed' not in res[0]
    md_kw = dict(temperature=300.0, friction=0.01, seed=3)
    ref = model.calc.md_many(*_md_args(systems), DT, 4, **md_kw)
    for fl in (None, nothing):
        res = model.calc.md_many(*_md_args(systems), DT, 4, fixed_list=fl, **md_kw)
        _same_dicts(res, ref)


@pytest.mark.parametrize('d3_term', ['host', 'device'])
def test_d3_sum_relaxes_under_a_mask(model, d3_term):   # noqa: F811
    from sevennet_amd.d3 import SevenNetD3Calculator
    calc = SevenNetD3Calculator((model.cfg, model.sd), file_type='model_instance', device=DEV, **D3_CUT)
    systems = _cells()[:1]
    held = _held(_cells())[0]
    res = calc.relax_many(*_args(systems), fmax=FMAX, steps=200, d3_term=d3_term, fixed_list=_masks(_cells())[:1])
    r = res[0]
    assert r['converged'] and 5 < r['n_steps'] < 200
    assert np.array_equal(r['positions'][held], systems[0][1][held]) and np.array_equal(r['fixed'], held)
    one = calc.compute(_args(systems)[0][0], r['positions'], systems[0][2], systems[0][3])
    fm_free = np.sqrt((np.where(held, 0.0, one['forces']) ** 2).sum(1).max())
    print(f'D3 {d3_term}: n_steps {r["n_steps"]}, max|F| free {fm_free:.5f} eV/A')
    assert fm_free < FMAX + 2e-5 * max(1.0, np.abs(one['forces']).max())
    assert np.abs(r['forces'] - one['forces']).max() <= 2e-5 * max(1.0, np.abs(one['forces']).max())   # model + D3, held atoms too


# ------------------------------------------------------------------------------------------------ md_many on a model
MD_STEPS = 20


@pytest.mark.parametrize('friction', [0.01, 0.0], ids=['langevin', 'nve'])
def test_md_many_holds_what_it_is_told_to_hold(model, friction):   # noqa: F811
    systems = _cells()
    held, masks = _held(systems), _masks(systems)
    vels = _start_velocities(systems) if friction == 0.0 else None   # NVE: the caller's velocities, held components not 0
    kw = dict(temperature=300.0, friction=friction, seed=3, velocities=vels, traj_every=1)
    res = model.calc.md_many(*_md_args(systems), DT, MD_STEPS, fixed_list=masks, **kw)
    for b, (types, pos, cell, pbc) in enumerate(systems):
        r = res[b]
        assert np.array_equal(r['fixed'], held[b])
        assert np.array_equal(r['positions'][held[b]], pos[held[b]]) and not r['velocities'][held[b]].any()
        assert all(np.array_equal(frame[held[b]], pos[held[b]]) for frame in r['trajectory'])
        assert r['velocities'][~held[b]].all() and (r['positions'][~held[b]] != pos[~held[b]]).all()
        dof = 3 * len(pos) - held[b].sum()
        assert np.array_equal(r['temperature'], 2.0 * r['e_kin'] / (dof * md_ref.KB)) and r['e_kin'].shape == (MD_STEPS + 1,)
        assert abs(r['e_kin'][-1] - md_ref.kinetic_energy(MASS_OF[types], r['velocities'])) <= 1e-12 * r['e_kin'][-1]
        if vels is None:   # drawn under the mask: dof kT / 2 exactly, so the first sample is the temperature asked for
            assert abs(r['temperature'][0] - 300.0) <= 1e-9
        else:
            v0 = np.where(held[b], 0.0, vels[b])
            assert abs(r['e_kin'][0] - md_ref.kinetic_energy(MASS_OF[types], v0)) <= 1e-12 * r['e_kin'][0]
    # a masked system run alone, under the id it had in the batch, equals itself inside the batch bit for bit
    b = 1
    alone = model.calc.md_many(*_md_args(systems[b:b + 1]), DT, MD_STEPS, fixed_list=masks[b:b + 1], system_ids=[b],
                               **dict(kw, velocities=None if vels is None else vels[b:b + 1]))
    for k in ('positions', 'velocities', 'e_kin', 'e_pot', 'temperature', 'trajectory'):
        assert np.array_equal(alone[0][k], res[b][k]), k
    if friction == 0.0:
        # the first steps follow the restatement driven by the fp64 oracle, within what a force error at the 1e-4 eV/A bar displaces
        n_first = 4
        for b, (types, pos, cell, pbc) in enumerate(systems):
            hold = (held[b].astype(int) << np.arange(3)).sum(1)
            o = fixed_ref.md_run(pos, lambda p, s=(types, cell, pbc): _oracle(model, s[0], p, s[1], s[2]), hold, MASS_OF[types], DT, n_first, vels[b])
            for k in range(n_first + 1):
                err = np.abs(res[b]['trajectory'][k] - o['traj'][k]).max()
                assert err <= _position_bound(k * DT), (b, k, err)
            print(f'cell {b}: max |dx| after {n_first} steps {err:.3e} A (bound {_position_bound(n_first * DT):.3e}), moved '
                  f'{np.abs(o["traj"][-1] - pos).max():.3e} A')


def test_md_many_atoms_reads_constraints_and_refuses_a_pressure(model):   # noqa: F811
    from test_md_batch_gpu import _Atoms
    from test_relax_gpu import Z

    class Fix:
        def __init__(self, **d):
            self.d = d

        def todict(self):
            return self.d
    systems = _cells()[:2]
    vels = _start_velocities(systems)
    atoms = [_Atoms(np.array(Z)[s[0]], s[1], s[2], s[3], MASS_OF[s[0]], v) for s, v in zip(systems, vels)]
    atoms[0].constraints = [Fix(name='FixAtoms', kwargs=dict(indices=[0, 2, 4, 6]))]
    atoms[1].constraints = [Fix(name='FixCartesian', kwargs=dict(a=list(range(8)), mask=[False, False, True]))]
    res = model.calc.md_many_atoms(atoms, DT, 3)
    ref = model.calc.md_many(*_md_args(systems), DT, 3, velocities=vels, fixed_list=_masks(_cells())[:2])
    for a, r, q, s in zip(atoms, res, ref, systems):
        assert np.array_equal(r['positions'], q['positions']) and np.array_equal(a.get_positions(), r['positions'])
        assert np.array_equal(a.get_positions()[r['fixed']], s[1][r['fixed']]) and not a.get_velocities()[r['fixed']].any()
    with pytest.raises(ValueError, match='fixed_list with pressure'):
        model.calc.md_many_atoms(atoms, DT, 3, pressure=0.0, compressibility=50.0)
