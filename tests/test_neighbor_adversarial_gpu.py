"""GPU: the device cell list (snet_neighbor.hip behind build_graph_gpu) and the batched list (snet_batch.hip behind
build_batch_graph, with its routing to the cell list and to the host list) against the brute-force list of tests/nl_ref.py on
the adversarial case table: strongly sheared and left-handed cells, atoms many lattice vectors outside the cell, atoms exactly on
cell faces, face distances at rc (k -+ 1e-3), rc / h on both sides of the 64-image routing boundary, skewed slabs and wires, one
atom in a thin cell, pairs at rc (1 -+ 1e-6).

Per case: the set of (center, src, shift) equals the reference's exactly (the table has no borderline pair -- asserted in
tests/test_nl_ref_cpu.py and again here -- so no pair is left out of any comparison); row_ptr / center form a valid CSR;
edge_vec equals the reference's fp64 vector rounded to fp32 within rc * 2^-23, one fp32 ulp at the cutoff (both sides round an
fp64 difference whose last bits may differ: the builders wrap the positions or add the image in another order).  Without shifts the
multiset of (center, src) is compared and the vectors are matched to their nearest reference vector within the same bound."""
import numpy as np
import pytest
import torch

from nl_ref import RC, adversarial_cases, brute_force_list

pytestmark = pytest.mark.gpu

CASES = adversarial_cases()
TOL = RC * 2.0 ** -23
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def reference():
    ref = {c.name: brute_force_list(c.pos, c.cell, c.pbc, RC) for c in CASES}
    assert all(len(r[3]) == 0 for r in ref.values())   # no borderline pair anywhere: every comparison below is complete
    return ref


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _rows_diff(got, want):
    g, w = set(map(tuple, got.tolist())), set(map(tuple, want.tolist()))
    return f'{len(got)} edges, {len(want)} expected; extra {sorted(g - w)[:5]}, missing {sorted(w - g)[:5]}'


def _check_csr(n, row_ptr, center, src, a0=0):
    """row_ptr / center describe the same CSR over atoms [a0, a0 + n) and every source is one of them"""
    assert row_ptr.shape == (n + 1,) and (np.diff(row_ptr) >= 0).all()
    assert np.array_equal(center, a0 + np.repeat(np.arange(n), np.diff(row_ptr)))
    assert len(src) == len(center) == row_ptr[-1] - row_ptr[0]
    assert ((src >= a0) & (src < a0 + n)).all()


def _check_edges(case, ref, center, src, shifts, ev, what):
    """one system's edges (indices relative to the system) against the reference"""
    ei, rv, rs, _ = ref
    want32 = rv.astype(np.float32).astype(np.float64)
    ev = ev.astype(np.float64)
    tag = f'{case.name} / {what}'
    if shifts is not None:
        got = np.concatenate([center[:, None], src[:, None], shifts], 1).astype(np.int64)
        want = np.concatenate([ei.T, rs], 1)
        og, ow = np.lexsort(got.T[::-1]), np.lexsort(want.T[::-1])
        assert got.shape == want.shape and np.array_equal(got[og], want[ow]), f'{tag}: {_rows_diff(got, want)}'
        err = np.abs(ev[og] - want32[ow]).max(initial=0.0)
        assert err <= TOL, f'{tag}: edge_vec off by {err:.3e} A (bound {TOL:.3e})'
    else:
        got, want = np.stack([center, src], 1).astype(np.int64), ei.T
        og = np.lexsort((ev[:, 2], ev[:, 1], ev[:, 0], got[:, 1], got[:, 0]))
        ow = np.lexsort((want32[:, 2], want32[:, 1], want32[:, 0], want[:, 1], want[:, 0]))
        got, gv, want, wv = got[og], ev[og], want[ow], want32[ow]
        assert got.shape == want.shape and np.array_equal(got, want), f'{tag}: {_rows_diff(got, want)}'
        bad = np.abs(gv - wv).max(1, initial=0.0) > TOL
        # vectors that tie within an ulp in x may sort differently: match those groups by nearest neighbour, one to one
        for c, s in set(map(tuple, got[bad].tolist())):
            m = (got[:, 0] == c) & (got[:, 1] == s)
            d = np.abs(gv[m][:, None, :] - wv[m][None, :, :]).max(-1)
            near = d.argmin(1)
            assert sorted(near.tolist()) == list(range(m.sum())) and d.min(1).max() <= TOL, \
                f'{tag}: vectors of pair ({c}, {s}) off by {d.min(1).max():.3e} A (bound {TOL:.3e})'
    listed = set(zip(center.tolist(), src.tolist()))
    assert all(p in listed for p in case.must_list) and not any(p in listed for p in case.must_not_list), tag


# ------------------------------------------------------------------------------------------------ the device cell list
@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_cell_list_equals_brute_force(case, reference):
    from sevennet_amd.neighbor_gpu import build_graph_gpu, gpu_neighbor_supported
    if not gpu_neighbor_supported(case.cell, case.pbc, RC, case.pos):
        assert case.name == 'reach_64p5'      # the only case beyond the cell list's 64 images; it refuses loudly
        with pytest.raises(RuntimeError):
            build_graph_gpu(case.types, case.pos, case.cell, RC, device=DEV, pbc=case.pbc)
        return
    n = len(case.pos)
    for with_shifts in (True, False):
        g = build_graph_gpu(case.types, case.pos, case.cell, RC, device=DEV, with_shifts=with_shifts, share_pairs=False, pbc=case.pbc)
        torch.cuda.synchronize()
        rp, cen, src, ev = _host(g.row_ptr), _host(g.center), _host(g.src), _host(g.edge_vec)
        assert g.n_local == n and g.n_edges == len(cen) == reference[case.name][0].shape[1], (g.n_edges, reference[case.name][0].shape)
        _check_csr(n, rp, cen, src)
        assert ev.dtype == np.float32 and ev.shape == (g.n_edges, 3)
        _check_edges(case, reference[case.name], cen, src, _host(g.shifts) if with_shifts else None, ev,
                     f'cell list, shifts {with_shifts}')
        assert np.array_equal(_host(g.types), case.types)
        # the source grouping the force kernels read: eperm sorts the edges by source, col_ptr counts them
        cp, ep = _host(g.col_ptr), _host(g.eperm)
        assert np.array_equal(np.diff(cp), np.bincount(src, minlength=n)) and np.array_equal(np.sort(ep), np.arange(g.n_edges))
        assert (np.diff(src[ep]) >= 0).all()


# ------------------------------------------------------------------------------------------------ the batched list
def _orders():
    return {'table': list(range(len(CASES))), 'shuffled': np.random.default_rng(0).permutation(len(CASES)).tolist()}


@pytest.mark.parametrize('with_shifts', [True, False])
@pytest.mark.parametrize('max_atoms', [2048, 32])
@pytest.mark.parametrize('order', ['table', 'shuffled'])
def test_batched_list_equals_brute_force(order, max_atoms, with_shifts, reference):
    """all cases in ONE heterogeneous batch.  max_atoms = 2048: every case in the batched kernel but reach_64p5, which goes to the
    host list; max_atoms = 32: the 216-atom cells go through the device cell list and are spliced in"""
    from sevennet_amd.batch import build_batch_graph, classify_systems
    cases = [CASES[k] for k in _orders()[order]]
    cells, pbcs = np.stack([c.cell for c in cases]), np.array([c.pbc for c in cases])
    kind = classify_systems(np.array([len(c.pos) for c in cases]), cells, pbcs, RC, max_atoms)
    want_kind = [2 if c.name == 'reach_64p5' else (1 if len(c.pos) > max_atoms else 0) for c in cases]
    assert kind.tolist() == want_kind
    assert set(want_kind) == ({0, 1, 2} if max_atoms == 32 else {0, 2})
    g = build_batch_graph([c.types for c in cases], [c.pos for c in cases], cells, pbcs, RC, 2, device=DEV, with_shifts=with_shifts,
                          share_pairs=False, max_atoms=max_atoms)
    torch.cuda.synchronize()
    sp = g.seg_ptr_host
    assert sp.tolist() == np.concatenate([[0], np.cumsum([len(c.pos) for c in cases])]).tolist()
    rp, cen, src, ev = _host(g.row_ptr), _host(g.center), _host(g.src), _host(g.edge_vec)
    sh = _host(g.shifts) if with_shifts else None
    assert (g.shifts is not None) == with_shifts
    _check_csr(g.n_local, rp, cen, src)
    assert g.n_edges == rp[-1] == sum(reference[c.name][0].shape[1] for c in cases)
    for b, c in enumerate(cases):
        a0, a1, e0, e1 = sp[b], sp[b + 1], rp[sp[b]], rp[sp[b + 1]]
        assert ((src[e0:e1] >= a0) & (src[e0:e1] < a1)).all(), c.name          # no edge crosses systems
        _check_edges(c, reference[c.name], cen[e0:e1] - a0, src[e0:e1] - a0, None if sh is None else sh[e0:e1], ev[e0:e1],
                     f'batch {order}, max_atoms {max_atoms}, shifts {with_shifts}')
        assert np.array_equal(_host(g.types)[a0:a1], c.types)
    cp, ep = _host(g.col_ptr), _host(g.eperm)
    assert np.array_equal(np.diff(cp), np.bincount(src, minlength=g.n_local)) and (np.diff(src[ep]) >= 0).all()


def test_pair_exactly_at_the_cutoff_is_not_listed():
    """d^2 < rc^2, strictly: the image at exactly rc (exact in fp64 in every order of operations, see nl_ref.EXACT_CUTOFF_CASE) is
    left out by the cell list and by the batched list"""
    from nl_ref import EXACT_CUTOFF_CASE as c
    from sevennet_amd.batch import build_batch_graph
    from sevennet_amd.neighbor_gpu import build_graph_gpu
    want = [[-1, 0, 0], [1, 0, 0]]
    g = build_graph_gpu(c.types, c.pos, c.cell, RC, device=DEV, with_shifts=True, share_pairs=False, pbc=c.pbc)
    assert sorted(_host(g.shifts).tolist()) == want
    g = build_batch_graph([c.types, c.types], [c.pos, c.pos], np.stack([c.cell, c.cell]), [True] * 3, RC, 2, device=DEV, with_shifts=True,
                          share_pairs=False)
    assert sorted(_host(g.shifts).tolist()) == sorted(want + want)
    assert np.array_equal(np.abs(_host(g.edge_vec)), np.abs(np.array(want + want, np.float32) * np.float32(RC / 2)))


def test_batched_list_takes_device_positions(reference):
    """positions that live on the device (what relax_many hands over every step): the same graph as from host arrays"""
    from sevennet_amd.batch import build_batch_graph
    cases = [c for c in CASES if c.name != 'reach_64p5']
    args = (np.stack([c.cell for c in cases]), np.array([c.pbc for c in cases]), RC, 2)
    pos = torch.as_tensor(np.concatenate([c.pos for c in cases])).to(DEV)
    types = torch.as_tensor(np.concatenate([c.types for c in cases])).to(DEV)
    g = build_batch_graph(types, pos, *args, n_atoms=[len(c.pos) for c in cases], device=DEV, with_shifts=True, share_pairs=False)
    h = build_batch_graph([c.types for c in cases], [c.pos for c in cases], *args, device=DEV, with_shifts=True, share_pairs=False)
    for k in ('row_ptr', 'center', 'src', 'edge_vec', 'shifts', 'col_ptr', 'eperm'):
        assert torch.equal(getattr(g, k), getattr(h, k)), k
    sp, rp = g.seg_ptr_host, _host(g.row_ptr)
    for b, c in enumerate(cases):
        assert rp[sp[b + 1]] - rp[sp[b]] == reference[c.name][0].shape[1], c.name
