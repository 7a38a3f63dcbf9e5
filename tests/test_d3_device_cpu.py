"""CPU: the host side of the device-resident D3 term -- the `d3_term` keyword of SevenNetD3Calculator, the `provides_virial`
marker through relax_batch's argument check and batch.BatchForces, the virial convention helper and the two new C-ABI entry
points.  The term itself runs HIP kernels only and is covered on the GPU (test_d3_device_gpu.py)."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_relax_cpu import _NoDeviceEngine, _two_systems

ONE = ([[14]], [np.zeros((1, 3))], np.eye(3)[None] * 6.0, [True] * 3)


def _bare_calc():
    from sevennet_amd.d3 import SevenNetD3Calculator
    return object.__new__(SevenNetD3Calculator)   # (the checks below come before the calculator's engines are looked at)


@pytest.mark.parametrize('bad', ['hip', 'Device', None, True])
def test_d3_term_is_validated(bad):
    calc = _bare_calc()
    with pytest.raises(ValueError, match='d3_term'):
        calc.relax_many(*ONE, d3_term=bad)
    with pytest.raises(ValueError, match='d3_term'):
        calc.md_many(*ONE[:2], [[28.0]], *ONE[2:], 1.0, 2, d3_term=bad)
    with pytest.raises(ValueError, match='d3_term'):
        calc.relax_many(*ONE, relax_cell=True, d3_term=bad)


def test_relax_cell_with_the_host_term_raises_and_names_the_device_term():
    calc = _bare_calc()
    for kw in ({}, dict(d3_term='host')):
        with pytest.raises(ValueError, match='no virial') as e:
            calc.relax_many(*ONE, relax_cell=True, **kw)
        assert "d3_term='device'" in str(e.value)
    with pytest.raises(AttributeError):   # the device term passes this check and goes on to the engines, which this stand-in lacks
        calc.relax_many(*ONE, relax_cell=True, d3_term='device')


class _Marked:
    provides_virial = True

    def __call__(self, pos, seg_ptr, ids, cells_dev=None):
        raise AssertionError('called before the input was validated')


def test_a_marked_extra_passes_the_argument_check_of_relax_batch():
    """the check that follows it (an open axis) is reached with the marker, and not with a plain callable"""
    from sevennet_amd.relax import relax_batch
    types, pos, _, _ = _two_systems()
    cells, pbcs = np.stack([np.eye(3) * 6.0] * 2), np.array([[True] * 3, [True, True, False]])
    run = lambda extra: relax_batch(_NoDeviceEngine(), types, pos, cells, pbcs, cutoff=5.0, relax_cell=True, extra=extra)   # noqa: E731
    with pytest.raises(ValueError, match='system 1: relax_cell needs a cell periodic'):
        run(_Marked())
    with pytest.raises(ValueError, match='no virial'):
        run(lambda *a: None)
    unmarked = _Marked()
    unmarked.provides_virial = False
    with pytest.raises(ValueError, match='no virial'):
        run(unmarked)


def test_batch_forces_keeps_the_virial_of_a_triple_and_still_returns_four_values(monkeypatch):
    import torch
    from sevennet_amd import batch
    n_atoms, seen = np.array([2, 1, 3]), []
    engine = SimpleNamespace(dev=torch.device('cpu'), spec=SimpleNamespace(num_species=2), needs_species_rows=False,
                             compute=lambda g, want_atomic_virial=False: {'forces': torch.zeros(g.n, 3)})

    def graph(ty, pos, cells, pbcs, cutoff, ns, n_atoms=None, device=None, species_rows=False, cells_dev=None):
        return SimpleNamespace(n=int(pos.shape[0]), seg_ptr_host=np.concatenate([[0], np.cumsum(n_atoms)]))
    monkeypatch.setattr(batch, 'build_batch_graph', graph)

    class Triple:
        provides_virial = True

        def __call__(self, pos, seg_ptr, ids, cells_dev=None):
            seen.append(cells_dev)
            b = len(ids)
            return np.ones((int(seg_ptr[-1]), 3)), np.arange(b, dtype=float), np.arange(6.0 * b).reshape(b, 6) + 100.0 * ids[0]

    args = (np.zeros(6, np.int64), n_atoms, np.stack([np.eye(3) * 6.0] * 3), np.ones((3, 3), bool), 5.0)
    forces = batch.BatchForces(engine, *args, extra=Triple())
    assert forces.virial_extra is None
    cells_dev = torch.arange(18.0, dtype=torch.float64).reshape(2, 9)
    out = forces(torch.zeros(4, 3, dtype=torch.float64), ids=[1, 2], cells_dev=cells_dev)
    assert len(out) == 4 and seen[-1] is cells_dev
    g, res, fx, ex = out
    assert fx.shape == (4, 3) and fx.dtype == torch.float64 and ex.tolist() == [0.0, 1.0]
    v = forces.virial_extra
    assert v.dtype == torch.float64 and v.shape == (2, 6) and v.is_contiguous()
    assert np.array_equal(v.numpy(), np.arange(12.0).reshape(2, 6) + 100.0)
    assert len(forces(torch.zeros(6, 3, dtype=torch.float64), with_extra=False)) == 4 and forces.virial_extra is None   # not a stale one
    # the two older contracts: bare forces, and (forces, energies) -- called without cells_dev, no virial kept
    for extra, has_e in ((lambda pos, sp, ids: np.ones((int(sp[-1]), 3)), False),
                         (lambda pos, sp, ids: (np.ones((int(sp[-1]), 3)), np.zeros(len(ids))), True)):
        forces = batch.BatchForces(engine, *args, extra=extra)
        g, res, fx, ex = forces(torch.zeros(6, 3, dtype=torch.float64), cells_dev=torch.zeros(3, 9, dtype=torch.float64))
        assert fx.shape == (6, 3) and (ex is not None) == has_e and forces.virial_extra is None


def test_fire_cell_loop_reads_the_virial_with_a_default():
    """the stand-in force objects of the existing tests have no `virial_extra`"""
    import inspect
    from sevennet_amd import relax
    assert "getattr(forces, 'virial_extra', None)" in inspect.getsource(relax.fire_cell_loop)


def test_stress_to_virial_on_a_hand_made_tensor():
    """stress = dE/d strain / V with entries xx 1, yy 2, zz 3, xy 4, xz 5, yz 6 and V = 2: the engine's order is xx,yy,zz,xy,yz,zx
    and its sign stress = -virial / V; cellrelax_ref.virial_matrix reads the result back as the symmetric matrix -V stress"""
    import cellrelax_ref
    from sevennet_amd.batch import virial_to_stress, voigt_to_3x3
    from sevennet_amd.d3 import stress_to_virial
    s = np.array([[1.0, 4.0, 5.0], [4.0, 2.0, 6.0], [5.0, 6.0, 3.0]])
    w = stress_to_virial(s, 2.0)
    assert w.tolist() == [-2.0, -4.0, -6.0, -8.0, -12.0, -10.0]
    assert np.array_equal(cellrelax_ref.virial_matrix(w), -2.0 * s)
    cell = np.diag([1.0, 1.0, 2.0])   # volume 2: the model side's conversion undoes it
    assert np.array_equal(voigt_to_3x3(virial_to_stress(w[None], cell[None])[0]), s)
    many = stress_to_virial(np.stack([s, 2.0 * s]), np.array([2.0, 0.5]))
    assert many.shape == (2, 6) and np.array_equal(many[0], w) and np.array_equal(many[1], 0.5 * w)


def test_the_two_entry_points_are_bound():
    from sevennet_amd import _lib
    assert len(_lib.SIGNATURES['snet_d3_plan'][1]) == 9 and len(_lib.SIGNATURES['snet_d3_compute_device'][1]) == 10
