"""CPU: what sevennet_amd.fd keeps of the unchanged copies of a plan (BaseCopies) is, system for system, what batch.batch_results
gives for a graph of those systems alone -- whichever call and position their copies were evaluated at -- and the check of the
copies a writer refused raises the drivers' message.  Torch CPU tensors stand in for the device's."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

N_AT = np.array([1, 3, 2], np.int64)
# per call: the copies in order, each (system, is it the unchanged copy).  The unchanged copies are spread over two calls, not in
# system order, the one of system 2 behind another copy; the last call holds none.
CALLS = [[(0, False), (2, True), (1, False)], [(2, False), (0, True), (1, True)], [(1, False), (0, False)]]


def _numbers(rng, n):
    """what an engine call gives for one copy of n atoms (dtypes as HipForceEngine.compute), its edge counts and extra forces"""
    return dict(energy=rng.normal(0.0, 3.0), virial=rng.normal(0.0, 1.0, 6), forces=rng.normal(0.0, 1.0, (n, 3)).astype(np.float32),
                atomic_energy=rng.normal(0.0, 1.0, n).astype(np.float32), atomic_virial=rng.normal(0.0, 1.0, (n, 6)).astype(np.float32),
                edges=rng.integers(0, 9, n), fx=rng.normal(0.0, 0.1, (n, 3)))


def _graph_and_output(copies):
    """(g, out, fx) of a force call over `copies` (a list of `_numbers`)"""
    n = np.array([len(c['edges']) for c in copies], np.int64)
    g = SimpleNamespace(seg_ptr_host=np.concatenate([[0], np.cumsum(n)]),
                        row_ptr=torch.as_tensor(np.concatenate([[0], np.cumsum(np.concatenate([c['edges'] for c in copies]))]).astype(np.int32)))
    cat = lambda k: torch.as_tensor(np.concatenate([c[k] for c in copies]))   # noqa: E731
    out = dict(energy_per_system=torch.as_tensor(np.array([c['energy'] for c in copies])),
               virial_per_system=torch.as_tensor(np.stack([c['virial'] for c in copies])), forces=cat('forces'),
               atomic_energy=cat('atomic_energy'), atomic_virial=cat('atomic_virial'))
    return g, out, cat('fx')


@pytest.fixture(scope='module')
def case():
    rng = np.random.default_rng(0)
    true = [_numbers(rng, int(k)) for k in N_AT]
    cells = rng.normal(0.0, 1.0, (3, 3, 3)) + 4.0 * np.eye(3)
    calls = []
    for copies in CALLS:
        call = SimpleNamespace(base=[(j, b) for j, (b, is_base) in enumerate(copies) if is_base])
        calls.append((call,) + _graph_and_output([true[b] if is_base else _numbers(rng, int(N_AT[b])) for b, is_base in copies]))
    g, out, _ = _graph_and_output(true)
    return SimpleNamespace(true=true, cells=cells, calls=calls, g=g, out=out)


def _same(got, want):
    assert type(got) is type(want)
    if isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    else:
        assert got == want


@pytest.mark.parametrize('energies_key', ['atomic_energies', 'energies'])
@pytest.mark.parametrize('want_atomic_virial', [False, True])
def test_base_copies_are_batch_results(case, energies_key, want_atomic_virial):
    from sevennet_amd.batch import batch_results
    from sevennet_amd.fd import BaseCopies
    base = BaseCopies(want_atomic_virial)
    for call, g, out, fx in case.calls:
        base(call, g, out, fx)
    assert len(base.kept) == 2   # (a call without an unchanged copy keeps nothing)
    got = base.results(N_AT, case.cells) if energies_key == 'energies' else base.results(N_AT, case.cells, energies_key)
    want = batch_results(case.g, case.out, case.cells, want_atomic_virial)
    assert len(got) == len(want) == 3
    for b in range(3):
        want[b][energies_key] = want[b].pop('energies')
        assert ('stresses' in got[b]) == want_atomic_virial
        assert set(got[b]) == set(want[b]), b
        for key in want[b]:
            _same(got[b][key], want[b][key])


def test_base_copies_keep_the_extra_forces_only_where_asked_and_given(case):
    from sevennet_amd.fd import BaseCopies
    for keep_extra, give in ((True, True), (True, False), (False, True)):
        base = BaseCopies(keep_extra=keep_extra)
        for call, g, out, fx in case.calls:
            base(call, g, out, fx if give else None)
        got = base.results(N_AT, case.cells)
        for b in range(3):
            assert ('forces_extra' in got[b]) == (keep_extra and give)
            if keep_extra and give:
                _same(got[b]['forces_extra'], case.true[b]['fx'])


def test_refused_copies_raise_the_drivers_message():
    from sevennet_amd.elastic import el_strain
    from sevennet_amd.fd import check_refused, refused_count
    from sevennet_amd.vib import vib_displace
    count = refused_count([torch.zeros(3, dtype=torch.int32), torch.tensor([0, 1, 1], dtype=torch.int32)])
    assert count.dtype == torch.float64 and count.shape == (1,) and count.item() == 2.0
    with pytest.raises(RuntimeError) as e:
        check_refused(count.numpy()[-1], vib_displace)
    assert str(e.value) == 'snet_vib_displace refused 2 copies of the plan: its descriptors do not fit the systems'
    with pytest.raises(RuntimeError) as e:
        check_refused(5.0, el_strain)
    assert str(e.value) == 'snet_el_strain refused 5 copies of the plan: its descriptors do not fit the systems'
    check_refused(0.0, vib_displace)
    check_refused(refused_count([torch.zeros(4, dtype=torch.int32)]).numpy()[-1], el_strain)
