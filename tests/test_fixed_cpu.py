"""CPU: atoms and components held fixed in relax_many / md_many -- the parser of `fixed_list`, the adapter that reads the
constraints of ASE-like objects, the refusals of the drivers (before any device work), the four masked entry points of the C
ABI, and the fp64 restatement of the masked steps (fixed_ref): that it is the unmasked restatement under an all-zero mask, and
that it relaxes a harmonic well with the held components bit-unchanged."""
from types import SimpleNamespace

import numpy as np
import pytest

import cellrelax_ref
import fixed_ref
import md_ref
import relax_ref


# ------------------------------------------------------------------------------------------------ the parser
def test_hold_masks_takes_every_stated_form():
    from sevennet_amd.fixed import held_components, hold_masks
    n_at = [3, 2, 4, 1, 2]
    comp = np.array([[True, False, False], [False, True, True]])
    hold = hold_masks([np.array([True, False, True]), comp, [3, 0], None, np.zeros(2, bool)], n_at)
    assert hold.dtype == np.int32 and hold.tolist() == [7, 0, 7, 1, 6, 7, 0, 0, 7, 0, 0, 0]
    assert held_components(hold).tolist()[3:5] == comp.tolist() and held_components(hold).dtype == bool
    # lists, tuples, numpy integers of any width, an index given twice, torch tensors
    import torch
    assert hold_masks(([True, False, True], comp.tolist(), np.array([3, 0, 3], np.uint8), None, None), n_at).tolist() == hold.tolist()
    assert hold_masks([torch.tensor([True, False, True]), torch.tensor(comp), torch.tensor([0, 3]), None, None], n_at).tolist() == hold.tolist()
    # nothing held is None: no argument, all None, empty index lists, all-false masks of either shape
    assert hold_masks(None, n_at) is None
    assert hold_masks([None] * 5, n_at) is None
    assert hold_masks([[], np.zeros((2, 3), bool), np.zeros(0, np.int64), np.zeros(1, bool), None], n_at) is None
    assert hold_masks([], []) is None


@pytest.mark.parametrize('fixed_list, match', [
    ([None, None], 'fixed_list has 2 entries but there are 3 systems'),
    (np.zeros(3, bool), 'one entry per system'),
    ([np.zeros(2, bool), None, None], r'system 0: a fixed mask of shape \(3,\)'),
    ([None, np.zeros((2, 2), bool), None], r'system 1: a fixed mask of shape \(2,\) .* or \(2, 3\)'),
    ([None, None, np.zeros((3, 4), bool)], 'system 2: a fixed mask of shape'),
    ([[3], None, None], 'system 0: fixed atom index 3 is out of range'),
    ([None, [-1], None], 'system 1: fixed atom index -1 is out of range'),
    ([None, None, [0.5, 1.0]], 'system 2: fixed atoms are given as'),
    ([None, None, [[0, 1]]], 'system 2: fixed atoms are given as'),
    ([np.array([0, None], object), None, None], 'system 0: .*objects'),
])
def test_hold_masks_names_the_system(fixed_list, match):
    from sevennet_amd.fixed import hold_masks
    with pytest.raises(ValueError, match=match):
        hold_masks(fixed_list, [3, 2, 4])


# ------------------------------------------------------------------------------------------------ the adapter
class _Constraint:
    def __init__(self, name, **kwargs):
        self.d = dict(name=name, kwargs=kwargs)

    def todict(self):
        return self.d


class _Atoms:
    """what relax_many_atoms / md_many_atoms read from and write to an ASE Atoms"""

    def __init__(self, n, constraints='absent'):
        self.n = n
        if constraints != 'absent':
            self.constraints = constraints

    def get_atomic_numbers(self):
        return np.full(self.n, 14)

    def get_positions(self):
        return np.arange(3.0 * self.n).reshape(self.n, 3)

    def get_masses(self):
        return np.full(self.n, 28.0855)

    def get_cell(self):
        return np.eye(3) * 9.0

    def get_pbc(self):
        return np.ones(3, bool)

    def set_positions(self, pos):
        self.pos = pos

    def set_velocities(self, vel):
        self.vel = vel


class _Recorder:
    """a calculator whose relax_many / md_many record their keywords"""

    def __init__(self):
        from sevennet_amd.atoms import ManyAtomsMixin
        self.kw = None
        self.mixin = ManyAtomsMixin

    def _results(self, numbers):
        return [dict(positions=np.zeros((len(z), 3)), velocities=np.zeros((len(z), 3))) for z in numbers]

    def relax_many(self, numbers, positions, cells, pbcs, fmax, steps, **kw):
        self.kw = kw
        return self._results(numbers)

    def md_many(self, numbers, positions, masses, cells, pbcs, dt, steps, **kw):
        self.kw = kw
        return self._results(numbers)

    def relax(self, atoms, **kw):
        return self.mixin.relax_many_atoms(self, atoms, **kw)

    def md(self, atoms, **kw):
        return self.mixin.md_many_atoms(self, atoms, 1.0, 2, temperature=300.0, **kw)


@pytest.mark.parametrize('surface', ['relax', 'md'])
def test_adapters_read_the_constraints(surface):
    calc = _Recorder()
    run = getattr(calc, surface)
    atoms = [_Atoms(4, [_Constraint('FixAtoms', indices=[0, 2])]),
             _Atoms(3, [_Constraint('FixCartesian', a=[1], mask=[False, False, True]), _Constraint('FixCartesian', a=2, mask=(True, True, False)),
                        _Constraint('FixAtoms', indices=np.array([0]))]),
             _Atoms(2), _Atoms(2, [])]
    run(atoms)
    fl = calc.kw['fixed_list']
    assert len(fl) == 4 and fl[2] is None and fl[3] is None
    assert fl[0].tolist() == [[True] * 3, [False] * 3, [True] * 3, [False] * 3]
    assert fl[1].tolist() == [[True] * 3, [False, False, True], [True, True, False]]
    from sevennet_amd.fixed import hold_masks
    assert hold_masks(fl, [4, 3, 2, 2]).tolist() == [7, 0, 7, 0, 7, 4, 3, 0, 0, 0, 0]
    # the caller's fixed_list takes precedence over the objects'
    mine = [[1], None, None, None]
    run(atoms, fixed_list=mine)
    assert calc.kw['fixed_list'] is mine
    # no constraints attribute, empty constraints, constraints that hold nothing: no fixed_list is passed on
    run([_Atoms(2), _Atoms(3, []), _Atoms(2, [_Constraint('FixAtoms', indices=[])])])
    assert 'fixed_list' not in calc.kw
    # any other constraint is refused by name, never dropped
    with pytest.raises(ValueError, match="system 1: constraint 'FixBondLength' is not supported"):
        run([_Atoms(2), _Atoms(3, [_Constraint('FixAtoms', indices=[0]), _Constraint('FixBondLength', a1=0, a2=1)])])
    with pytest.raises(ValueError, match="system 0: constraint 'object' is not supported"):
        run([_Atoms(2, [object()])])
    with pytest.raises(ValueError, match='system 0: constraint FixAtoms: atom index 5 is out of range'):
        run([_Atoms(2, [_Constraint('FixAtoms', indices=[5])])])


# ------------------------------------------------------------------------------------------------ the refusals
class _NoDeviceEngine:
    spec = SimpleNamespace(num_species=2)

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


def _two_cells():
    types = [np.array([0, 1]), np.array([1, 0, 0])]
    pos = [np.array([[0.0, 0, 0], [1.2, 0, 0]]), np.array([[0.0, 0, 0], [1.5, 0.1, 0], [0.2, 1.6, 0.3]])]
    return types, pos, np.stack([np.eye(3) * 6.0] * 2), np.ones((2, 3), bool)


def test_refusals_come_before_any_device_work(no_device):
    from sevennet_amd.md import md_batch
    from sevennet_amd.relax import relax_batch
    types, pos, cells, pbcs = _two_cells()
    masses = [np.full(2, 28.0855), np.full(3, 15.999)]
    partial = [None, np.array([[True, True, True], [False, False, False], [True, False, True]])]
    with pytest.raises(ValueError, match='system 1: relax_cell holds whole atoms only, and atom 2'):
        relax_batch(_NoDeviceEngine(), types, pos, cells, pbcs, cutoff=5.0, relax_cell=True, fixed_list=partial)
    for bad, match in (([None], 'fixed_list has 1 entries'), ([None, [3]], 'system 1: fixed atom index 3')):
        with pytest.raises(ValueError, match=match):
            relax_batch(_NoDeviceEngine(), types, pos, cells, pbcs, cutoff=5.0, fixed_list=bad)
        with pytest.raises(ValueError, match=match):
            md_batch(_NoDeviceEngine(), types, pos, masses, cells, pbcs, cutoff=5.0, dt=1.0, steps=2, temperature=300.0, fixed_list=bad)
    with pytest.raises(ValueError, match='fixed_list with pressure'):
        md_batch(_NoDeviceEngine(), types, pos, masses, cells, pbcs, cutoff=5.0, dt=1.0, steps=2, temperature=300.0, pressure=0.0,
                 compressibility=50.0, fixed_list=[[0], None])


def test_the_masked_entry_points_are_the_base_ones_plus_the_mask():
    import ctypes as C
    import inspect
    from sevennet_amd import _lib, md, relax
    for base in ('snet_fire_step', 'snet_fire_cell_step', 'snet_mdb_step', 'snet_mdb_init_velocities'):
        res, args = _lib.SIGNATURES[base]
        res_f, args_f = _lib.SIGNATURES[base + '_fixed']
        assert res_f is res and len(args_f) == len(args) + 1
        assert args_f[:-2] == args[:-1] and args_f[-2] is C.c_void_p and args_f[-1] is args[-1]   # ..., hold, stream
    assert 'snet_mdb_npt_step_fixed' not in _lib.SIGNATURES and _lib.ABI_VERSION == 4
    for fn in (relax.fire_step, relax.fire_cell_step, relax.fire_loop, relax.fire_cell_loop, md.md_step, md.init_velocities, md.md_loop):
        assert inspect.signature(fn).parameters['hold'].default is None, fn.__name__
    for fn in (relax.relax_batch, md.md_batch):
        assert inspect.signature(fn).parameters['fixed_list'].default is None


# ------------------------------------------------------------------------------------------------ the restatement
def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) else a[k] == b[k], k


def test_an_all_zero_mask_is_the_unmasked_restatement():
    rng = np.random.default_rng(0)
    n = 7
    zero = np.zeros(n, int)
    s = relax_ref.fire_init(rng.normal(0, 0.5, (n, 3)))
    for it in range(12):
        f = (-2.0 * s['pos']).astype(np.float32)
        (a, wa), (b, wb) = fixed_ref.fire_step(s, f, zero, 0.01), relax_ref.fire_step(s, f, 0.01)
        _same(a, b)
        assert wa == wb
        s = b
    c = cellrelax_ref.cell_fire_init(rng.normal(0, 0.5, (n, 3)), np.eye(3) * 4.0 + rng.normal(0, 0.1, (3, 3)), cell0=np.eye(3) * 4.0)
    for it in range(6):
        f, w = -2.0 * c['pos'], rng.normal(0, 1.0, 6)
        (a, wa), (b, wb) = fixed_ref.cell_fire_step(c, f, w, zero, 0.01), cellrelax_ref.cell_fire_step(c, f, w, 0.01)
        _same(a, b)
        assert wa['branch'] == wb['branch'] and wa['fm'] == wb['fm']
        c = b
    mass = rng.choice([1.008, 15.999, 28.0855], n)
    m = md_ref.md_init(rng.normal(0, 0.5, (n, 3)), rng.normal(0, 0.01, (n, 3)))
    c1, c2 = md_ref.langevin_coefficients(0.1, 0.5)
    for phase in (2, 3, 3, 0, 1):
        f = -2.0 * m['pos']
        (a, ea), (b, eb) = fixed_ref.md_step(m, f, zero, mass, 0.02, 0.5, c1, c2, 5, 3, phase), md_ref.md_step(m, f, mass, 0.02, 0.5, c1, c2, 5, 3, phase)
        _same(a, b)
        assert ea == eb
        m = b
    for remove_com in (True, False):
        assert np.array_equal(fixed_ref.init_velocities(mass, zero, 0.02, 5, 3, remove_com), md_ref.init_velocities(mass, 0.02, 5, 3, remove_com))


def test_the_restated_masked_steps_hold_what_they_should():
    rng = np.random.default_rng(1)
    n = 9
    hold = rng.integers(0, 8, n)
    hold[0], hold[1] = 7, 0
    held = fixed_ref.components(hold)
    assert held[0].all() and not held[1].any() and 0 < held.sum() < 3 * n
    # FIRE on a harmonic well: converges on the free components, the held ones keep their bits, NaN forces on them go nowhere
    x0 = rng.normal(0, 0.5, (n, 3))

    def force(pos, poison=False):
        f = -3.0 * pos
        return np.where(held, np.nan, f) if poison else f
    s, log = fixed_ref.fire_relax(x0, force, hold, 1e-3, 400)
    sp, _ = fixed_ref.fire_relax(x0, lambda p: force(p, True), hold, 1e-3, 400)
    assert s['active'] == 0 and 5 < s['n_steps'] < 400 and {w['branch'] for w in log} >= {'uphill', 'downhill'}
    assert np.array_equal(s['pos'][held], x0[held]) and not s['vel'][held].any()
    assert np.abs(s['pos'][~held]).max() < 1e-3 / 3.0 and np.abs(x0[held]).max() > 0.1   # free: at the minimum; held: far from it
    assert np.array_equal(s['pos'], sp['pos']) and np.array_equal(s['vel'], sp['vel']) and s['n_steps'] == sp['n_steps']
    free_only, _ = relax_ref.fire_relax(x0, lambda p: np.where(held, 0.0, -3.0 * p), 1e-3, 400)[:2]
    assert free_only['n_steps'] == s['n_steps']   # (the well is separable: the same path as a well without the held springs)
    # everything held: converged at once, no step counted
    s, log = fixed_ref.fire_relax(x0, force, np.full(n, 7), 1e-3, 10)
    assert s['active'] == 0 and s['n_steps'] == 0 and len(log) == 1 and log[0]['fm'] == 0.0 and np.array_equal(s['pos'], x0)
    # MD: held positions keep their bits, held velocities are 0 after any phase that stores, free components are md_ref's bits
    mass = rng.choice([1.008, 15.999, 28.0855], n)
    m = md_ref.md_init(x0, rng.normal(0, 0.01, (n, 3)))
    c1, c2 = md_ref.langevin_coefficients(0.1, 0.5)
    a, ea = fixed_ref.md_step(m, force(x0, True), hold, mass, 0.02, 0.5, c1, c2, 5, 3, 3)
    b, eb = md_ref.md_step(m, force(x0), mass, 0.02, 0.5, c1, c2, 5, 3, 3)
    assert np.array_equal(a['pos'][held], x0[held]) and not a['vel'][held].any()
    assert np.array_equal(a['pos'][~held], b['pos'][~held]) and np.array_equal(a['vel'][~held], b['vel'][~held])
    v_free = np.where(held, 0.0, m['vel'] + 0.25 * md_ref.ACC * force(x0) / mass[:, None])
    assert abs(ea - md_ref.kinetic_energy(mass, v_free)) <= 1e-14 * ea and ea < eb
    same, e0 = fixed_ref.md_step(m, force(x0), hold, mass, 0.02, 0.5, c1, c2, 5, 3, 0)
    assert np.array_equal(same['vel'], m['vel']) and np.array_equal(same['pos'], m['pos'])
    # the draw: held components 0, KE = dof kT / 2, no centre-of-mass shift; nothing free: zeros
    kT = md_ref.KB * 300.0
    v = fixed_ref.init_velocities(mass, hold, kT, 5, 3)
    dof = 3 * n - held.sum()
    assert not v[held].any() and v[~held].all() and abs(md_ref.kinetic_energy(mass, v) - 0.5 * dof * kT) <= 1e-13 * dof * kT
    raw = fixed_ref.init_velocities(mass, hold, kT, 5, 3, remove_com=False)
    assert np.array_equal(raw[~held], md_ref.init_velocities(mass, kT, 5, 3, remove_com=False)[~held])
    ratio = v[~held] / raw[~held]
    assert np.abs(ratio - ratio[0]).max() <= 1e-14 * abs(ratio[0])   # a scaling and nothing else
    assert not fixed_ref.init_velocities(mass[:1], [7], kT, 5, 3).any() and not np.isnan(fixed_ref.init_velocities(mass, np.full(n, 7), kT, 5, 3)).any()
    # the cell step: a held atom keeps its fractional coordinates while the cell moves
    c = cellrelax_ref.cell_fire_init(x0, np.eye(3) * 4.0 + rng.normal(0, 0.1, (3, 3)), cell0=np.eye(3) * 4.0)
    whole = np.where(np.arange(n) % 2 == 0, 7, 0)
    frac0 = c['pos'] @ np.linalg.inv(c['cell'])
    for it in range(5):
        c, what = fixed_ref.cell_fire_step(c, -2.0 * c['pos'], np.array([3.0, -2.0, 1.0, 0.5, -0.4, 0.2]) * n, whole, 0.01)
        assert what['branch'] is not None
    frac = c['pos'] @ np.linalg.inv(c['cell'])
    assert np.abs(frac - frac0)[whole == 7].max() < 1e-12 and np.abs(frac - frac0)[whole == 0].max() > 1e-3
    assert not c['vel'][whole == 7].any() and not np.array_equal(c['cell'], np.eye(3) * 4.0)
