"""CPU: host-side preparation of a batched D3 evaluation (sevennet_amd.d3.prepare_d3_batch): validation before any device
work, the molecule box of D3Engine.compute per system, and the flat layout snet_d3_compute_batch reads."""
import numpy as np
import pytest

from test_d3_cpu import H2O_POS, NACL, h2o_box

RTHR, CNTHR = 9000.0, 1600.0


def _systems():
    rng = np.random.default_rng(1)
    tri = np.array([[7.0, 0.4, 0.0], [0.3, 6.5, 0.5], [0.2, 0.6, 8.0]])
    return [
        (NACL['numbers'], NACL['positions'], NACL['cell'], NACL['pbc']),
        ([8, 1, 1], H2O_POS, np.zeros((3, 3)), [False] * 3),
        ([6, 8, 1, 14, 8, 22, 1, 1, 79], rng.uniform(-0.3, 1.2, (9, 3)) @ tri, tri, [True, True, False]),
        ([1], [[0.3, -0.2, 0.1]], np.zeros((3, 3)), [False] * 3),
    ]


def _prep(systems, **kw):
    from sevennet_amd.d3 import prepare_d3_batch
    return prepare_d3_batch([s[0] for s in systems], [s[1] for s in systems], np.array([s[2] for s in systems], float),
                            np.array([s[3] for s in systems]), RTHR, CNTHR, **kw)


def test_layout_and_molecule_box():
    systems = _systems()
    bt = _prep(systems)
    n = [len(s[0]) for s in systems]
    assert bt.atom_ptr.dtype == np.int64 and bt.atom_ptr.tolist() == np.concatenate([[0], np.cumsum(n)]).tolist()
    assert bt.numbers.dtype == np.int32 and bt.numbers.tolist() == sum([list(s[0]) for s in systems], [])
    assert bt.positions.dtype == np.float64 and bt.positions.shape == (sum(n), 3) and bt.positions.flags.c_contiguous
    assert np.array_equal(bt.positions, np.concatenate([np.asarray(s[1], float).reshape(-1, 3) for s in systems]))
    assert bt.cells.shape == (4, 3, 3) and bt.pbcs.dtype == np.int32 and bt.pbcs.shape == (4, 3)
    # periodic cells untouched; H2O gets exactly the reference's generated box, all axes periodic
    assert np.array_equal(bt.cells[0], np.asarray(NACL['cell'], float)) and bt.pbcs[0].tolist() == [1, 1, 1]
    assert np.array_equal(bt.cells[1], h2o_box()) and bt.pbcs[1].tolist() == [1, 1, 1]
    assert np.array_equal(bt.cells[2], systems[2][2]) and bt.pbcs[2].tolist() == [1, 1, 0]
    assert np.array_equal(bt.cells[3], np.eye(3) * (np.sqrt(9000.0) * 0.52917726 + 1.0))


def test_molecule_box_is_the_single_system_rule():
    from sevennet_amd.d3 import molecule_box
    cell, pbc = molecule_box(H2O_POS, np.zeros((3, 3)), [False] * 3, RTHR, CNTHR)
    assert np.array_equal(cell, h2o_box()) and pbc.tolist() == [True] * 3
    cell, pbc = molecule_box(H2O_POS, np.zeros((3, 3)), [False] * 3, 400.0, 2500.0)   # the longer of the two cutoffs
    assert np.allclose(np.diag(cell) - (H2O_POS.max(0) - H2O_POS.min(0)), 50.0 * 0.52917726 + 1.0)
    cell, pbc = molecule_box(H2O_POS, NACL['cell'], [True, False, True], RTHR, CNTHR)
    assert np.array_equal(cell, np.asarray(NACL['cell'], float)) and pbc.tolist() == [True, False, True]


def test_flat_and_per_system_forms_agree():
    from sevennet_amd.d3 import prepare_d3_batch
    systems = _systems()
    a = _prep(systems)
    b = prepare_d3_batch(np.concatenate([np.asarray(s[0]) for s in systems]),
                         np.concatenate([np.asarray(s[1], float).reshape(-1, 3) for s in systems]),
                         np.array([s[2] for s in systems], float), np.array([s[3] for s in systems]), RTHR, CNTHR,
                         n_atoms=[len(s[0]) for s in systems])
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    # one pbc row for all systems
    c = _prep([(s[0], s[1], s[2], [True] * 3) for s in systems[:1]] * 3)
    d = prepare_d3_batch([s[0] for s in systems[:1]] * 3, [s[1] for s in systems[:1]] * 3, np.array([NACL['cell']] * 3, float),
                         [True] * 3, RTHR, CNTHR)
    for x, y in zip(c, d):
        assert np.array_equal(x, y)


@pytest.mark.parametrize('bad_z,what', [(0, 'Z = 0'), (95, 'Z = 95'), (-3, 'Z = -3')])
def test_rejects_unknown_elements(bad_z, what):
    systems = _systems()
    systems[2] = ([6, 8, bad_z] + list(systems[2][0][3:]), systems[2][1], systems[2][2], systems[2][3])
    with pytest.raises(ValueError, match=f'system 2: {what}'):
        _prep(systems)


def test_rejects_malformed_batches():
    from sevennet_amd.d3 import prepare_d3_batch
    systems = _systems()
    cells = np.array([s[2] for s in systems], float)
    pbcs = np.array([s[3] for s in systems])
    nums, poss = [s[0] for s in systems], [s[1] for s in systems]
    with pytest.raises(ValueError, match='empty batch'):
        prepare_d3_batch([], [], np.zeros((0, 3, 3)), np.zeros((0, 3), bool), RTHR, CNTHR)
    with pytest.raises(ValueError, match='system 1 has no atoms'):
        prepare_d3_batch([nums[0], [], nums[2]], [poss[0], np.zeros((0, 3)), poss[2]], cells[[0, 1, 2]], pbcs[[0, 1, 2]], RTHR, CNTHR)
    with pytest.raises(ValueError, match='4 type arrays but 3 position arrays'):
        prepare_d3_batch(nums, poss[:3], cells, pbcs, RTHR, CNTHR)
    with pytest.raises(ValueError, match='system 2: 9 types but 8 positions'):
        prepare_d3_batch(nums, poss[:2] + [poss[2][:8]] + poss[3:], cells, pbcs, RTHR, CNTHR)
    with pytest.raises(ValueError, match='n_atoms sums to'):
        prepare_d3_batch(np.concatenate([np.asarray(z) for z in nums]), np.concatenate([np.reshape(p, (-1, 3)) for p in poss]),
                         cells, pbcs, RTHR, CNTHR, n_atoms=[2, 3, 9, 2])
    with pytest.raises(ValueError, match='cells of shape'):
        prepare_d3_batch(nums, poss, cells[:3], pbcs, RTHR, CNTHR)
    with pytest.raises(ValueError, match='pbc of shape'):
        prepare_d3_batch(nums, poss, cells, pbcs[:2], RTHR, CNTHR)


def test_rejects_singular_periodic_cells():
    from sevennet_amd.d3 import prepare_d3_batch
    systems = _systems()
    flat = np.array([[5.0, 0.0, 0.0], [0.0, 5.0, 0.0], [0.0, 0.0, 0.0]])   # a slab with a zero row: no box rule applies
    systems[3] = ([1, 1], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.74]], flat, [True, True, False])
    with pytest.raises(ValueError, match='system 3: singular cell'):
        _prep(systems)
    collinear = np.array([[3.0, 0.0, 0.0], [6.0, 0.0, 0.0], [0.0, 0.0, 4.0]])
    with pytest.raises(ValueError, match='system 0: singular cell'):
        prepare_d3_batch([[14]], [[[0.0, 0.0, 0.0]]], collinear[None], [True] * 3, RTHR, CNTHR)
