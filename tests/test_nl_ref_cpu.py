"""CPU: the brute-force neighbor list of tests/nl_ref.py against hand-counted answers, the zero-borderline condition of the
adversarial case table, and the host KD-tree list (sevennet_amd.neighbor.neighbor_list) against the brute-force list on every
case -- index for index, with the caller's image shifts.  The GPU builders meet the same table in
tests/test_neighbor_adversarial_gpu.py."""
import numpy as np
import pytest

from nl_ref import RC, adversarial_cases, brute_force_list, image_range

CASES = adversarial_cases()


def _rows(ei, sh):
    return np.concatenate([np.asarray(ei).T, np.asarray(sh)], 1).astype(np.int64)


# ------------------------------------------------------------------------------------------------ hand-counted answers
def test_simple_cubic_has_six_neighbors():
    """a < rc < a sqrt(2): the six <100> neighbors and nothing else, whether the cell holds 1 atom (all of them self images) or 27"""
    a, rc = 3.0, 3.7
    ei, ev, sh, border = brute_force_list([[0.2, 0.1, -0.3]], np.eye(3) * a, [True] * 3, rc)
    assert ei.shape == (2, 6) and (ei == 0).all() and len(border) == 0
    assert sorted(map(tuple, sh.tolist())) == sorted([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
    assert np.array_equal(ev, sh * a)
    g = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing='ij'), -1).reshape(-1, 3) * a
    ei, ev, sh, border = brute_force_list(g, np.eye(3) * 3 * a, [True] * 3, rc)
    assert ei.shape == (2, 27 * 6) and (np.bincount(ei[0]) == 6).all() and (np.bincount(ei[1]) == 6).all()
    assert np.allclose(np.linalg.norm(ev, axis=1), a, rtol=0, atol=1e-12)
    assert np.allclose(g[ei[1]] - g[ei[0]] + sh @ (np.eye(3) * 3 * a), ev, rtol=0, atol=1e-12)


def test_dimer_in_an_open_box():
    pos = np.array([[0.0, 0.0, 0.0], [0.0, 3.0, 4.0 - 1e-3]])
    for cell in (np.zeros((3, 3)), np.diag([2.0, 2.0, 2.0])):   # an open axis is not imaged, whatever its cell row
        ei, ev, sh, _ = brute_force_list(pos, cell, [False] * 3, 5.0)
        assert ei.T.tolist() == [[0, 1], [1, 0]] and (sh == 0).all()
        assert np.array_equal(ev, np.array([pos[1] - pos[0], pos[0] - pos[1]]))
    ei, _, _, _ = brute_force_list(pos + [[0, 0, 0], [0, 0, 2e-3]], np.zeros((3, 3)), [False] * 3, 5.0)
    assert ei.shape == (2, 0)
    # periodic along x only, period 2: the dimer and the images of both atoms at +-2, +-4 (4^2 + 25 - ... > 25 for the partner)
    ei, ev, sh, _ = brute_force_list(pos, [[2.0, 0, 0], [0, 0, 0], [0, 0, 0]], [True, False, False], 5.0)
    assert (sh[:, 1:] == 0).all()
    assert sorted(sh[(ei[0] == 0) & (ei[1] == 0), 0].tolist()) == [-2, -1, 1, 2]
    assert sorted(sh[(ei[0] == 0) & (ei[1] == 1), 0].tolist()) == [0]   # |(2, 3, 4 - 1e-3)| > 5


def test_one_atom_in_a_cell_of_height_rc_over_2p5():
    """4 self images along the thin axis (+-1, +-2; +-3 is at 1.2 rc), none along the wide ones"""
    rc = 5.0
    ei, ev, sh, border = brute_force_list([[7.0, -3.0, 0.5]], np.diag([rc / 2.5, 3 * rc, 4 * rc]), [True] * 3, rc)
    assert sorted(map(tuple, sh.tolist())) == [(-2, 0, 0), (-1, 0, 0), (1, 0, 0), (2, 0, 0)] and len(border) == 0
    # exactly on the cutoff (height rc / 2: the second image is AT rc): not listed, and reported as borderline
    ei, ev, sh, border = brute_force_list([[0.0, 0.0, 0.0]], np.diag([rc / 2, 3 * rc, 4 * rc]), [True] * 3, rc)
    assert sorted(sh[:, 0].tolist()) == [-1, 1]
    assert sorted(border[:, 2].tolist()) == [-2, 2]


def test_image_range_covers_far_atoms():
    cell = np.diag([4.0, 50.0, 50.0])
    pos = np.array([[0.1, 1, 1], [0.3 + 4.0 * 17, 1, 1]])
    assert image_range(pos, cell, [True] * 3, 5.0)[0] >= 17 + 2
    ei, ev, sh, _ = brute_force_list(pos, cell, [True] * 3, 5.0)
    assert sorted(sh[(ei[0] == 0) & (ei[1] == 1), 0].tolist()) == [-18, -17, -16]   # 0.2 - 4, 0.2, 0.2 + 4


def test_host_list_pair_exactly_at_the_cutoff():
    """the one geometry whose distance IS the cutoff in every order of operations (atom at the origin, cell height rc / 2: every
    product and sum is exact in fp64): the convention is d^2 < rc^2, so the second image is not listed.  Kept out of the case
    table, whose comparisons rest on having no pair within 1e-9 rc^2 of the cutoff."""
    from sevennet_amd.neighbor import neighbor_list
    from nl_ref import EXACT_CUTOFF_CASE as c
    ei, ev, sh, border = brute_force_list(c.pos, c.cell, c.pbc, RC)
    assert sorted(sh[:, 0].tolist()) == [-1, 1] and len(border) == 2
    hi, hv, hs = neighbor_list(c.pos, c.cell, c.pbc, RC)
    assert sorted(hs.tolist()) == sorted(sh.tolist()) and (hi == 0).all()   # (the host list orders by (i, j) only)
    assert np.array_equal(hv, hs * (RC / 2))


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_is_what_it_claims():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert all(1 <= len(c.pos) <= 216 and len(c.types) == len(c.pos) for c in CASES)
    by = {c.name: c for c in CASES}
    assert np.linalg.det(by['shear_left_handed'].cell) < 0 < np.linalg.det(by['shear'].cell)
    inv = np.linalg.inv(by['shear'].cell)
    assert RC * np.linalg.norm(inv, axis=0).max() > 10          # strongly sheared: many images along one axis
    for name, lo in (('lattice_jumps', 2.5), ('lattice_jumps_1000', 999.0)):
        f = by[name].pos @ np.linalg.inv(by[name].cell)
        assert f.max() > lo and f.min() < -lo
    f = by['on_faces_orthogonal'].pos @ np.linalg.inv(by['on_faces_orthogonal'].cell)
    assert ((f < 0) & (f > -1e-16)).any() and (f == 0).any()
    assert ((f - np.floor(f)) == 1.0).any()                      # the wrap that yields 1.0
    for k in (1, 2, 3):
        for tag, s in (('below', -1), ('above', 1)):
            h = by[f'face_{k}rc_{tag}'].cell[0, 0]
            assert abs(h / RC - (k + s * 1e-3)) < 1e-12
    for tag, reach in (('63p5', 63.5), ('64p5', 64.5)):
        assert abs(RC * np.linalg.norm(np.linalg.inv(by[f'reach_{tag}'].cell)[:, 0]) - reach) < 1e-9
    for name in ('slab_skewed', 'wire_skewed'):
        c = by[name]
        assert not all(c.pbc) and all(np.count_nonzero(c.cell[k]) > 1 for k in range(3) if not c.pbc[k])


@pytest.fixture(scope='module')
def reference():
    return {c.name: brute_force_list(c.pos, c.cell, c.pbc, RC) for c in CASES}


def test_no_case_has_a_borderline_pair(reference):
    """the condition every comparison relies on: no pair within 1e-9 rc^2 of the cutoff, so no comparison leaves a pair out"""
    assert {name: len(r[3]) for name, r in reference.items() if len(r[3])} == {}


def test_constructed_pairs_at_the_cutoff(reference):
    seen = 0
    for c in CASES:
        ei = reference[c.name][0]
        listed = set(map(tuple, ei.T.tolist()))
        for p in c.must_list:
            assert p in listed, (c.name, p)
        for p in c.must_not_list:
            assert p not in listed, (c.name, p)
        seen += len(c.must_list) + len(c.must_not_list)
    assert seen >= 24
    d = np.linalg.norm(reference['cutoff_pairs_periodic'][1], axis=1)
    assert (np.abs(d / RC - 1) < 1.1e-6).sum() == 4   # two pairs at rc (1 - 1e-6), both directions, through a face


def test_reference_edges_are_consistent(reference):
    for c in CASES:
        ei, ev, sh, _ = reference[c.name]
        if len(c.pos) > 1 or all(c.pbc):
            assert ei.shape[1] > 0 or c.name in ('isolated_atom',), c.name
        # every edge has its reverse with the opposite shift and vector
        fwd = set(map(tuple, _rows(ei, sh).tolist()))
        assert fwd == set(map(tuple, _rows(ei[::-1], -sh).tolist())), c.name
        assert (np.einsum('ij,ij->i', ev, ev) < RC * RC).all()
    assert reference['single_atom_thin'][0].shape[1] > 20 and reference['isolated_atom'][0].shape[1] == 0


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_host_list_equals_brute_force(case, reference):
    """sevennet_amd.neighbor.neighbor_list: the same (i, j, S) rows in the same (i, j) order; edge_vec within 1e-9 A (the host
    list wraps the positions first: a round trip through fractional coordinates at |pos| up to 1000 lattice vectors costs
    1000 * 6 A * 2^-52 * a few operations ~ 1e-11 A)"""
    from sevennet_amd.neighbor import neighbor_list
    ei, ev, sh, border = reference[case.name]
    assert len(border) == 0
    hi, hv, hs = neighbor_list(case.pos, case.cell, case.pbc, RC)
    want, got = _rows(ei, sh), _rows(hi, hs)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert (np.diff(hi[0]) >= 0).all()                                  # sorted by center
    og, ow = np.lexsort(got.T[::-1]), np.lexsort(want.T[::-1])
    assert np.array_equal(got[og], want[ow])
    assert np.abs(hv[og] - ev[ow]).max(initial=0.0) < 1e-9
