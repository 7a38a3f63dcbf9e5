"""GPU: the force call of the batched drivers (sevennet_amd.batch.BatchForces) on the three small systems of helpers.py -- a
subset of the systems against compute_many bit for bit, the counters, the one `extra` contract, and relax_batch with an
`extra` that also returns energies."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import three_small_systems
from test_batch_gpu import Z, _calc

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def model():
    from sevennet_amd.batch import validate_batch_inputs
    from sevennet_amd.shapes import mini_sevennet_0_config
    calc, _, _ = _calc(mini_sevennet_0_config())
    systems = three_small_systems()
    inputs = validate_batch_inputs([s[0] for s in systems], [s[1] for s in systems], np.stack([s[2] for s in systems]),
                                   np.array([s[3] for s in systems]), calc.cutoff, calc.model.spec.num_species)
    return SimpleNamespace(calc=calc, systems=systems, inputs=inputs)


def _forces(model, extra=None):
    from sevennet_amd.batch import BatchForces
    types, _, n_at, cells, pbcs = model.inputs
    return BatchForces(model.calc.model, types, n_at, cells, pbcs, model.calc.cutoff, extra)


def _pos(model, ids):
    return torch.as_tensor(np.concatenate([model.systems[b][1] for b in ids])).to(DEV)


def test_a_subset_equals_compute_many_bit_for_bit(model):
    ids = [0, 2]
    forces = _forces(model)
    g, out, fx, ex = forces(_pos(model, ids), ids)
    assert fx is None and ex is None
    assert (forces.n_force_calls, forces.system_steps_evaluated) == (1, 2)
    sub = [model.systems[b] for b in ids]
    want = model.calc.compute_many([np.array(Z)[s[0]] for s in sub], [s[1] for s in sub], np.stack([s[2] for s in sub]),
                                   np.array([s[3] for s in sub]))
    assert g.seg_ptr_host.tolist() == [0, 2, 10]
    assert np.array_equal(out['forces'].cpu().numpy().astype(np.float64), np.concatenate([r['forces'] for r in want]))
    assert out['energy_per_system'].cpu().numpy().tolist() == [r['energy'] for r in want]
    forces(_pos(model, [0, 1, 2]))   # all systems: the default
    assert (forces.n_force_calls, forces.system_steps_evaluated) == (2, 5)


def test_the_extra_contract(model):
    ids = [2, 0]
    pos = _pos(model, ids)
    rng = np.random.default_rng(1)
    given_f, given_e = rng.normal(0, 1, (10, 3)), rng.normal(0, 1, 2).astype(np.float32)
    seen = []

    def on_the_host(p, seg_ptr, sys_ids):
        seen.append((p, seg_ptr, sys_ids))
        return given_f

    g, out, fx, ex = _forces(model, on_the_host)(pos, ids)
    p, seg_ptr, sys_ids = seen[0]
    assert p is pos and isinstance(seg_ptr, np.ndarray) and seg_ptr.dtype == np.int64 and seg_ptr.tolist() == [0, 8, 10]
    assert np.asarray(sys_ids).dtype == np.int64 and np.asarray(sys_ids).tolist() == ids
    assert ex is None and fx.dtype == torch.float64 and fx.is_contiguous() and fx.device == torch.device(DEV)
    assert np.array_equal(fx.cpu().numpy(), given_f)
    on_device = torch.as_tensor(given_f.astype(np.float32).T.copy()).to(DEV).T   # fp32, not contiguous
    assert not on_device.is_contiguous()
    g, out, fx, ex = _forces(model, lambda *a: (on_device, given_e))(pos, ids)
    assert fx.dtype == torch.float64 and fx.is_contiguous() and fx.device == torch.device(DEV)
    assert np.array_equal(fx.cpu().numpy(), given_f.astype(np.float32).astype(np.float64))
    assert ex.dtype == torch.float64 and tuple(ex.shape) == (2,) and ex.device == torch.device(DEV)
    assert np.array_equal(ex.cpu().numpy(), given_e.astype(np.float64))
    g, out, fx, ex = _forces(model, on_the_host)(pos, ids, with_extra=False)   # the caller asks for none
    assert fx is None and ex is None and len(seen) == 1


def test_relax_batch_takes_forces_with_energies(model):
    """an `extra` that returns (forces, energies) relaxes to the same bits as the same forces alone"""
    from sevennet_amd.relax import relax_batch
    types, pos, n_at, cells, pbcs = model.inputs
    pull = lambda p, seg_ptr, ids: -0.05 * p   # noqa: E731
    both = lambda p, seg_ptr, ids: (pull(p, seg_ptr, ids), np.arange(len(ids), dtype=np.float64))   # noqa: E731
    run = lambda extra: relax_batch(model.calc.model, types, pos, cells, pbcs, cutoff=model.calc.cutoff, fmax=1e-4, steps=6,   # noqa: E731
                                    repack_below=1.0, extra=extra, n_atoms=n_at)
    (a, info_a), (b, info_b) = run(pull), run(both)
    assert info_a == info_b and info_a['fire_launches'] >= 1
    for x, y in zip(a, b):
        assert np.array_equal(x['positions'], y['positions']) and x['n_steps'] == y['n_steps']
    assert any(x['n_steps'] > 0 for x in a)
