"""CPU: host side of batched evaluation -- input validation, system-order bookkeeping, concat_graphs on CPU tensors, and the
Voigt / 3x3 stress conversion against hand-computed values."""
import numpy as np
import pytest
import torch

from sevennet_amd.batch import (BATCH_MAX_ATOMS, _normalize, classify_systems, concat_graphs, virial_to_stress,
                                voigt_to_3x3)
from sevennet_amd.engine import build_graph
from sevennet_amd.neighbor import diamond_cubic, neighbor_list

RC = 4.0


def _cpu_graph(pos, cell, pbc, types):
    ei, ev, sh = neighbor_list(pos, cell, pbc, RC)
    g = build_graph(types, ei, ev, device='cpu', num_species=0, share_pairs=False)
    g.shifts = torch.as_tensor(sh, dtype=torch.int32)
    return g, ei, ev, sh


def _systems():
    p1, c1 = diamond_cubic(5.431, (1, 1, 1), 0.05, 0)
    p2 = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.1], [0.9, 0.0, -0.3]])   # molecule, zero cell
    p3 = np.zeros((1, 3))                                                # isolated atom
    p4, c4 = diamond_cubic(5.431, (1, 1, 1), 0.08, 3)
    return [(p1, c1, [True] * 3, np.array([0, 1] * 4)), (p2, np.zeros((3, 3)), [False] * 3, np.array([1, 0, 0])),
            (p3, np.zeros((3, 3)), [False] * 3, np.array([1])), (p4, c4, [True, True, False], np.zeros(8, np.int64))]


def test_validation_raises_value_error():
    pos = [np.zeros((2, 3)), np.ones((1, 3))]
    types = [np.zeros(2, np.int64), np.zeros(1, np.int64)]
    cells = np.zeros((2, 3, 3))
    with pytest.raises(ValueError, match='no atoms'):
        _normalize([np.zeros(0, np.int64)], [np.zeros((0, 3))], np.zeros((1, 3, 3)), [False] * 3, None)
    with pytest.raises(ValueError, match='empty batch'):
        _normalize([], [], np.zeros((0, 3, 3)), [False] * 3, None)
    with pytest.raises(ValueError, match='types but'):
        _normalize([np.zeros(2, np.int64), np.zeros(2, np.int64)], pos, cells, [False] * 3, None)
    with pytest.raises(ValueError, match='position arrays'):
        _normalize(types, pos[:1], cells, [False] * 3, None)
    with pytest.raises(ValueError, match='n_atoms sums'):
        _normalize(np.zeros(3, np.int64), np.zeros((3, 3)), cells, [False] * 3, n_atoms=[2, 2])
    with pytest.raises(ValueError, match='no atoms'):
        _normalize(np.zeros(3, np.int64), np.zeros((3, 3)), np.zeros((3, 3, 3)), [False] * 3, n_atoms=[3, 0, 0])
    with pytest.raises(ValueError, match='cells of shape'):
        _normalize(types, pos, np.zeros((3, 3, 3)), [False] * 3, None)
    with pytest.raises(ValueError, match='pbc of shape'):
        _normalize(types, pos, cells, np.zeros((3, 3), bool), None)
    # flat and per-system input describe the same batch
    t1, p1, n1, c1, b1 = _normalize(types, pos, cells, [True, False, True], None)
    t2, p2, n2, c2, b2 = _normalize(np.concatenate(types), np.concatenate(pos), cells, [[True, False, True]] * 2, n_atoms=[2, 1])
    assert np.array_equal(t1, t2) and np.array_equal(p1, p2) and np.array_equal(n1, n2) and np.array_equal(b1, b2)
    assert b1.shape == (2, 3) and c1.shape == (2, 3, 3)


def test_unknown_species_raises_before_any_device_work():
    from sevennet_amd.batch import build_batch_graph
    with pytest.raises(ValueError, match='unknown species'):
        build_batch_graph([np.array([0, 5])], [np.zeros((2, 3))], np.zeros((1, 3, 3)), [False] * 3, RC, num_species=2, device='cpu')
    with pytest.raises(ValueError, match='unknown species'):
        build_batch_graph([np.array([-1])], [np.zeros((1, 3))], np.zeros((1, 3, 3)), [False] * 3, RC, num_species=2, device='cpu')


def test_classification_of_systems():
    cells = np.stack([np.eye(3) * 10, np.zeros((3, 3)), np.diag([10.0, 10.0, 0.01]), np.eye(3) * 10,
                      np.diag([10.0, 10.0, 0.0])])
    pbcs = np.array([[1, 1, 1], [0, 0, 0], [1, 1, 1], [1, 1, 1], [1, 1, 0]], bool)
    n = np.array([5, 3, 2, BATCH_MAX_ATOMS + 1, 4])
    kind = classify_systems(n, cells, pbcs, RC)
    # bulk and molecule: batched kernel; a periodic height of rc/400: host list; above the threshold: cell list;
    # a slab whose open axis has a zero cell row is padded like dataload.py:37-48
    assert kind.tolist() == [0, 0, 2, 1, 0]
    with pytest.raises(ValueError, match='singular cell'):
        classify_systems(np.array([2]), np.diag([10.0, 10.0, 0.0])[None], np.array([[1, 1, 1]], bool), RC)
    with pytest.raises(ValueError, match='singular cell'):   # degenerate rows on open axes are not padded (dataload.py)
        classify_systems(np.array([2]), np.array([[[1.0, 0, 0], [2.0, 0, 0], [0, 0, 1.0]]]), np.array([[0, 0, 0]], bool), RC)


def test_concat_graphs_on_cpu_keeps_order_and_offsets():
    systems = _systems()
    graphs, singles = [], []
    for pos, cell, pbc, types in systems:
        g, ei, ev, sh = _cpu_graph(pos, cell, pbc, types)
        graphs.append(g)
        singles.append((ei, ev, sh, types))
    b = concat_graphs(graphs, num_species=2, share_pairs=False)
    n_at = [len(s[0]) for s in systems]
    assert b.seg_ptr_host.tolist() == np.concatenate([[0], np.cumsum(n_at)]).tolist()
    assert b.seg_ptr.dtype == torch.int32 and b.seg_ptr.tolist() == b.seg_ptr_host.tolist()
    assert b.n_total == b.n_local == sum(n_at) and b.n_edges == sum(s[0].shape[1] for s in singles)
    rp, cen, src = b.row_ptr.numpy(), b.center.numpy(), b.src.numpy()
    assert rp[0] == 0 and rp[-1] == b.n_edges and (np.diff(rp) >= 0).all()
    assert (np.repeat(np.arange(b.n_local), np.diff(rp)) == cen).all()   # CSR by center
    for k, (ei, ev, sh, types) in enumerate(singles):   # system k: its own edges, offset, in order
        a0, a1 = b.seg_ptr_host[k], b.seg_ptr_host[k + 1]
        e0, e1 = rp[a0], rp[a1]
        assert np.array_equal(cen[e0:e1] - a0, ei[0]) and np.array_equal(src[e0:e1] - a0, ei[1])
        assert np.allclose(b.edge_vec[e0:e1].numpy(), ev, atol=1e-6)
        assert np.array_equal(b.shifts[e0:e1].numpy(), sh)
        assert np.array_equal(b.types[a0:a1].numpy(), types)
        assert ((src[e0:e1] >= a0) & (src[e0:e1] < a1)).all()   # no edge crosses systems
    # source grouping and species rows recomputed over the whole batch
    cp, ep = b.col_ptr.numpy(), b.eperm.numpy()
    assert np.array_equal(cp, np.concatenate([[0], np.cumsum(np.bincount(src, minlength=b.n_local))]))
    assert np.array_equal(src[ep], np.sort(src)) and sorted(ep.tolist()) == list(range(b.n_edges))
    t = b.types.numpy()
    for s in range(2):
        assert np.array_equal(b.species_rows[s].numpy(), np.nonzero(t == s)[0])
    # the isolated atom has no edges and still is one system
    a0 = b.seg_ptr_host[2]
    assert rp[a0 + 1] == rp[a0]
    with pytest.raises(ValueError):
        concat_graphs([])


def test_stress_conversion_by_hand():
    # engine virial order xx,yy,zz,xy,yz,zx; cell volume 2*3*4 = 24
    vir = np.array([[24.0, 48.0, 72.0, 2.4, 4.8, 7.2], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    cells = np.stack([np.diag([2.0, 3.0, 4.0]), np.zeros((3, 3))])
    s = virial_to_stress(vir, cells)
    # ASE Voigt xx,yy,zz,yz,xz,xy = -(virial / V)[[0,1,2,4,5,3]]
    assert np.allclose(s[0], [-1.0, -2.0, -3.0, -0.2, -0.3, -0.1])
    assert np.isnan(s[1]).all()   # zero volume: NaN, as SevenNetCalculator.compute
    m = voigt_to_3x3(s[0])
    assert np.allclose(m, [[-1.0, -0.1, -0.3], [-0.1, -2.0, -0.2], [-0.3, -0.2, -3.0]])
    t = voigt_to_3x3(torch.tensor(s[:1]))
    assert t.shape == (1, 3, 3) and np.allclose(t[0].numpy(), m)
    # the TorchSim mapping: stress = -voigt_6_to_full_3x3((virial / V)[[0,1,2,4,5,3]]) is the same tensor
    ts = -voigt_to_3x3(torch.tensor(vir[:1] / 24.0)[..., [0, 1, 2, 4, 5, 3]])
    assert np.allclose(ts[0].numpy(), m)


def test_system_of_at_the_ends_of_every_system():
    from sevennet_amd.batch import system_of
    a_ptr = np.array([0, 2, 3, 8, 9])   # systems of 2, 1, 5 and 1 atoms
    for b in range(4):
        assert system_of(a_ptr, a_ptr[b]) == b and system_of(a_ptr, a_ptr[b + 1] - 1) == b
    assert [system_of(a_ptr, i) for i in range(9)] == [0, 0, 1, 2, 2, 2, 2, 2, 3] and type(system_of(a_ptr, 4)) is int


def test_validate_batch_inputs_names_the_system():
    """the six messages of test_relax_cpu's bad-systems test, from the function itself"""
    from sevennet_amd.batch import validate_batch_inputs
    types = [np.array([0, 1]), np.array([1])]
    pos = [np.array([[0.0, 0, 0], [1.2, 0, 0]]), np.array([[0.0, 0, 0]])]
    cells = np.stack([np.eye(3) * 6.0, np.zeros((3, 3))])
    pbcs = np.array([[True] * 3, [False] * 3])
    v = lambda t=types, p=pos, c=cells, b=pbcs: validate_batch_inputs(t, p, c, b, 5.0, 2)   # noqa: E731
    with pytest.raises(ValueError, match='system 1: unknown species index 2'):
        v(t=[types[0], np.array([2])])
    with pytest.raises(ValueError, match='system 0: singular cell'):
        v(c=np.stack([np.diag([6.0, 6.0, 0.0]), np.zeros((3, 3))]))
    with pytest.raises(ValueError, match='system 1: 1 types but 2 positions'):
        v(p=[pos[0], np.zeros((2, 3))])
    with pytest.raises(ValueError, match='system 1 has no atoms'):
        v(t=[types[0], np.zeros(0, np.int64)], p=[pos[0], np.zeros((0, 3))])
    with pytest.raises(ValueError, match='system 0: non-finite position'):
        v(p=[np.array([[0.0, 0, 0], [np.nan, 0, 0]]), pos[1]])
    with pytest.raises(ValueError, match='empty batch'):
        v(t=[], p=[], c=np.zeros((0, 3, 3)), b=np.zeros((0, 3), bool))
    ty, p, n_at, c, b = v()   # and what it returns for a good batch
    assert ty.tolist() == [0, 1, 1] and ty.dtype == np.int64 and p.shape == (3, 3) and n_at.tolist() == [2, 1]
    assert c.shape == (2, 3, 3) and b.shape == (2, 3) and b.dtype == bool
