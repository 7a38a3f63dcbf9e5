"""CPU: batched FIRE relaxation -- input validation before any device work, the fp64 restatement of the step (relax_ref) pinned
to hand-computed values, and the repack bookkeeping.  The driver itself cannot run on CPU tensors (its neighbor build, engine
call and step are HIP kernels, and there is no CPU path), so the loop is covered on the GPU (test_relax_gpu.py); what is
host-only -- validation, the repack rule and its index arithmetic, the result layout -- is covered here."""
from types import SimpleNamespace

import numpy as np
import pytest

import relax_ref


class _NoDeviceEngine:
    """stands for a HipForceEngine in calls that must fail before they reach it: any use beyond spec.num_species is an error"""
    spec = SimpleNamespace(num_species=2)

    def __getattr__(self, name):
        raise AssertionError(f'the engine was touched ({name}) before the input was validated')


def _two_systems():
    types = [np.array([0, 1]), np.array([1])]
    pos = [np.array([[0.0, 0, 0], [1.2, 0, 0]]), np.array([[0.0, 0, 0]])]
    cells = np.stack([np.eye(3) * 6.0, np.zeros((3, 3))])
    pbcs = np.array([[True] * 3, [False] * 3])
    return types, pos, cells, pbcs


def _relax(**kw):
    from sevennet_amd.relax import relax_batch
    types, pos, cells, pbcs = _two_systems()
    args = dict(types=types, positions=pos, cells=cells, pbcs=pbcs, cutoff=5.0)
    args.update(kw)
    return relax_batch(_NoDeviceEngine(), args.pop('types'), args.pop('positions'), args.pop('cells'), args.pop('pbcs'), **args)


@pytest.mark.parametrize('kw, match', [
    (dict(fmax=-0.01), 'fmax'),
    (dict(fmax=float('nan')), 'fmax'),
    (dict(steps=-1), 'steps'),
    (dict(steps=2.5), 'steps'),
    (dict(repack_below=1.5), 'repack_below'),
    (dict(dt_start=0.0), 'dt_start'),
    (dict(dt_start=0.5, dt_max=0.1), 'dt_max'),
    (dict(f_inc=0.9), 'f_inc'),
    (dict(f_dec=1.0), 'f_dec'),
    (dict(alpha_start=0.0), 'alpha_start'),
    (dict(f_alpha=1.5), 'f_alpha'),
    (dict(max_step=-1.0), 'max_step'),
    (dict(n_min=-1), 'n_min'),
    (dict(timestep=0.1), 'timestep'),
    (dict(cutoff=0.0), 'cutoff'),
])
def test_bad_parameters_raise_before_any_device_work(kw, match):
    with pytest.raises(ValueError, match=match):
        _relax(**kw)


def test_bad_systems_raise_before_any_device_work_and_name_the_system():
    types, pos, cells, pbcs = _two_systems()
    with pytest.raises(ValueError, match='system 1: unknown species index 2'):
        _relax(types=[types[0], np.array([2])])
    with pytest.raises(ValueError, match='system 0: singular cell'):
        _relax(cells=np.stack([np.diag([6.0, 6.0, 0.0]), np.zeros((3, 3))]))
    with pytest.raises(ValueError, match='system 1: 1 types but 2 positions'):
        _relax(positions=[pos[0], np.zeros((2, 3))])
    with pytest.raises(ValueError, match='system 1 has no atoms'):
        _relax(types=[types[0], np.zeros(0, np.int64)], positions=[pos[0], np.zeros((0, 3))])
    with pytest.raises(ValueError, match='system 0: non-finite position'):
        _relax(positions=[np.array([[0.0, 0, 0], [np.nan, 0, 0]]), pos[1]])
    with pytest.raises(ValueError, match='empty batch'):
        _relax(types=[], positions=[], cells=np.zeros((0, 3, 3)), pbcs=np.zeros((0, 3), bool))


def test_batch_forces_is_constructed_without_any_device_work(monkeypatch):
    """BatchForces on the engine that may not be touched, with torch.cuda.device / current_stream / synchronize raising"""
    import torch
    from sevennet_amd.batch import BatchForces, validate_batch_inputs

    def touched(*a, **k):
        raise AssertionError('torch.cuda was touched by the constructor')
    for name in ('device', 'current_stream', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, touched)
    types, pos, cells, pbcs = _two_systems()
    ty, _, n_at, cells, pbcs = validate_batch_inputs(types, pos, cells, pbcs, 5.0, 2)
    forces = BatchForces(_NoDeviceEngine(), ty, n_at, cells, pbcs, 5.0, extra=lambda *a: None)
    assert (forces.n_force_calls, forces.system_steps_evaluated) == (0, 0)


def test_restatement_follows_the_rule_on_a_harmonic_well():
    """F = -k r with k = 1 from r0: step 0 has v = 0, so P = 0 and dt halves; then P > 0 until far beyond step n_min + 3 (the
    time integrated, < 0.5, is well short of the quarter period pi / 2), so n_pos counts up, and dt and alpha first change in the
    step that starts with n_pos = 6 > n_min"""
    r0 = np.array([[0.3, -0.2, 0.1], [0.0, 0.4, 0.0]])
    s = relax_ref.fire_init(r0)
    assert (s['dt'], s['alpha'], s['n_pos'], s['active'], s['n_steps']) == (0.1, 0.1, 0, 1, 0) and not s['vel'].any()
    want = [(0.05, 0.1, 0)] + [(0.05, 0.1, k) for k in range(1, 7)] + [(0.05 * 1.1, 0.1 * 0.99, 7)]
    assert len(want) == relax_ref.FIRE['n_min'] + 3
    for k, (dt, alpha, n_pos) in enumerate(want):
        before = s
        s, what = relax_ref.fire_step(s, -s['pos'], fmax=1e-3)
        assert (s['dt'], s['alpha'], s['n_pos'], s['n_steps']) == (dt, alpha, n_pos, k + 1), k
        assert what['branch'] == ('uphill' if k == 0 else 'downhill') and not what['clipped']
        if k == 0:   # v = dt F, r += dt v
            assert np.array_equal(s['vel'], 0.05 * -r0) and np.array_equal(s['pos'], r0 + 0.05 * (0.05 * -r0))
        else:        # F is antiparallel to r and v parallel to F: the mixing keeps |v|, so v' = v + dt F exactly in direction
            f = -before['pos']
            v_mix = 0.9 * before['vel'] + 0.1 * f / np.sqrt((f * f).sum()) * np.sqrt((before['vel'] ** 2).sum())
            assert np.allclose(s['vel'], v_mix + dt * f, rtol=1e-15, atol=0)
    # and it gets there
    s, log, dts = relax_ref.fire_relax(r0, lambda r: -r, fmax=1e-3, steps=500)
    assert s['active'] == 0 and log[-1]['fm'] < 1e-3 and s['n_steps'] == len(dts) == len(log) - 1 < 200
    assert max(dts) <= relax_ref.FIRE['dt_max']


def test_restatement_clips_the_step_and_freezes_converged_systems():
    r0 = np.array([[30.0, 0.0, 0.0]])
    s, what = relax_ref.fire_step(relax_ref.fire_init(r0), -100.0 * r0, fmax=0.05)   # dr = 0.05 * 0.05 * 3000 = 7.5 > 0.2
    assert what['clipped'] and abs(np.linalg.norm(s['pos'] - r0) - 0.2) < 1e-12 and s['vel'][0, 0] == 0.05 * -3000.0
    s0 = relax_ref.fire_init(r0)
    s1, what = relax_ref.fire_step(s0, np.full((1, 3), 0.01), fmax=0.05)               # |F| = 0.0173 < fmax
    assert s1['active'] == 0 and s1['n_steps'] == 0 and np.array_equal(s1['pos'], r0) and what['branch'] is None
    s2, _ = relax_ref.fire_step(s1, np.full((1, 3), 10.0), fmax=0.05)                  # inactive: untouched whatever the force
    assert s2 == {**s1, 'pos': s2['pos'], 'vel': s2['vel']} and np.array_equal(s2['pos'], r0)


def test_repack_rule():
    from sevennet_amd.relax import RepackBook
    w = RepackBook.wants_repack
    assert not w(8, 8, 1.0)          # nobody has finished
    assert w(7, 8, 1.0)              # repack_below = 1: as soon as one finishes
    assert not w(5, 8, 0.5) and w(4, 8, 0.5) and w(1, 8, 0.5)
    assert not w(0, 8, 0.5)          # nothing left: the loop ends instead
    assert not any(w(k, 8, 0.0) for k in range(9))   # switched off


def test_repack_bookkeeping_keeps_the_callers_order():
    """five systems of 2, 1, 3, 1, 2 atoms; systems 1 and 3 finish first, then 0, and 2 and 4 run into the step cap"""
    from sevennet_amd.relax import RepackBook
    n_atoms = np.array([2, 1, 3, 1, 2])
    book = RepackBook(n_atoms)
    pos = np.arange(9 * 3, dtype=np.float64).reshape(9, 3)    # row r belongs to the caller's atom r
    assert book.seg_ptr().tolist() == [0, 2, 3, 6, 7, 9]
    keep, rows = book.repack(pos, active=np.array([1, 0, 1, 0, 1]), n_steps=np.array([4, 4, 4, 2, 4]))
    assert keep.tolist() == [0, 2, 4] and rows.tolist() == [0, 1, 3, 4, 5, 7, 8] and book.ids.tolist() == [0, 2, 4]
    assert book.seg_ptr().tolist() == [0, 2, 5, 7]
    pos2 = pos[rows] + 100.0                                   # the shrunken batch moves on
    keep, rows2 = book.repack(pos2, active=np.array([0, 1, 1]), n_steps=np.array([9, 9, 9]))
    assert keep.tolist() == [1, 2] and rows2.tolist() == [2, 3, 4, 5, 6] and book.ids.tolist() == [2, 4]
    pos3 = pos2[rows2] + 100.0
    book.store(pos3, active=np.array([1, 1]), n_steps=np.array([12, 12]), only_finished=False)
    assert book.n_repacks == 2
    assert book.n_steps.tolist() == [9, 4, 12, 2, 12] and book.converged.tolist() == [True, True, False, True, False]
    final = np.concatenate(book.positions)
    moved = np.array([100.0, 100, 0, 200, 200, 200, 0, 200, 200])   # how far each of the caller's atoms travelled with its batch
    assert np.array_equal(final, pos + moved[:, None])


def test_result_layout():
    """attach_relaxed adds exactly positions / converged / n_steps, per system, as host values"""
    import torch
    from sevennet_amd.relax import attach_relaxed
    final = torch.arange(9, dtype=torch.float64).reshape(3, 3)
    res = attach_relaxed([{'energy': -1.0}, {'energy': -2.0}], final, np.array([0, 2, 3]), np.array([5, 0]), np.array([False, True]))
    assert [set(r) for r in res] == [{'energy', 'positions', 'converged', 'n_steps'}] * 2
    assert res[0]['positions'].shape == (2, 3) and res[1]['positions'].tolist() == [[6.0, 7.0, 8.0]]
    assert res[0]['positions'].dtype == np.float64 and type(res[0]['converged']) is bool and type(res[1]['n_steps']) is int
    assert (res[0]['converged'], res[0]['n_steps'], res[1]['converged'], res[1]['n_steps']) == (False, 5, True, 0)


def test_calculator_surfaces_exist():
    from sevennet_amd.calculator import SevenNetCalculator
    from sevennet_amd.d3 import SevenNetD3Calculator
    for cls in (SevenNetCalculator, SevenNetD3Calculator):
        assert callable(cls.relax_many) and callable(cls.relax_many_atoms)
    from sevennet_amd import _lib
    assert 'snet_fire_step' in _lib.SIGNATURES and len(_lib.SIGNATURES['snet_fire_step'][1]) == 24
