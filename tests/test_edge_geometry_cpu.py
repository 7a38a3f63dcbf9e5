"""CPU: the case table of tests/edge_cases.py holds what it says (so that no case can be dropped silently), the fp64 reference of
tests/edge_ref.py is finite on all of it and agrees with the engine's own harmonic polynomials, and the fp32 restatement of the
reference's modules stays inside the bounds this project asserts for the kernels.  The kernels meet the same table in
tests/test_edge_geometry_gpu.py."""
import numpy as np
import pytest
import torch

from edge_cases import (FORCE_SEG, LATTICE_SCALES, R_ON, RC, SIZES, edge_of_row_map, force_graph, lattice_edges, lattice_integers,
                        lattice_partner, length_fp32, params_table, radial_edges, radial_lengths, sized_edges)
from edge_ref import cached_reference, force_reference64

PARAMS = params_table()
GROUPS = ('lattice', 'radial')


def _norm64(v):
    return np.linalg.norm(np.asarray(v, np.float64), axis=1)


# ------------------------------------------------------------------------------------------------ the table itself
def test_lattice_set_is_complete_and_symmetric():
    ints, lat, partner = lattice_integers(), lattice_edges(), lattice_partner()
    assert ints.shape == (124, 3) and len({tuple(v) for v in ints.tolist()}) == 124 and np.abs(ints).max() == 2
    assert lat.shape == (248, 3) and lat.dtype == np.float32
    assert np.array_equal(lat[partner], -lat) and np.array_equal(partner[partner], np.arange(248))      # -v beside every v
    r = _norm64(lat)
    assert abs(r.min() - 0.37) < 1e-7 and abs(r.max() - 2 * 3 ** 0.5 * 1.3575) < 1e-6 and 4.70 < r.max() < 4.71
    # components exactly 0 or equal in magnitude, every sign pattern, whole shells of one fp32 |r|
    for k, s in enumerate(LATTICE_SCALES):
        block = lat[124 * k:124 * (k + 1)]
        assert set(np.unique(np.abs(block)).tolist()) == {0.0, float(np.float32(s)), float(np.float32(2 * s))}
        assert len({tuple(np.sign(v).tolist()) for v in block}) == 26
        assert len(np.unique(length_fp32(block))) == 9         # |n|^2 in {1, 2, 3, 4, 5, 6, 8, 9, 12}
    assert ((lat == 0).sum(1) == 2).sum() == 12 * 2 and ((lat == 0).sum(1) == 0).sum() == 64 * 2


def test_radial_set_reaches_both_ends_and_stops_at_the_cutoff():
    for rc, r_on in ((RC, R_ON), (6.0, 5.5)):
        r = radial_lengths(rc, r_on)
        on, c = np.float32(r_on), np.float32(rc)
        assert r.dtype == np.float32 and len(r) == 27 and len(np.unique(r)) == 27
        assert r[:3].tolist() == [np.float32(0.3), np.float32(0.4), 1.0]
        assert r[4] == on and np.nextafter(r[3], c) == on and np.nextafter(on, c) == r[5]          # r_on between its fp32 neighbours
        assert all(r[6 + i] == np.float32(rc * (1 - 2.0 ** -(4 + i))) for i in range(20))
        below = np.nextafter(c, np.float32(0))
        assert r[25] in (below, np.nextafter(below, np.float32(0))) and r[26] == c                 # within two ulps of r_c; r_c
        assert rc != RC or r[25] == below                                                          # (5 x 2^-23 is 1.25 ulps)
        vec = radial_edges(rc, r_on)
        assert vec.shape == (54, 3) and vec.dtype == np.float32
        assert np.array_equal(vec[:27], np.stack([0 * r, r, 0 * r], 1))                            # the polar axis, exactly
        assert np.array_equal(length_fp32(vec[:27]), r)
        assert (np.abs(_norm64(vec[27:]) / r.astype(np.float64) - 1) <= 2.0 ** -24).all()
        assert (vec[27:] != 0).all()


def test_nothing_lies_beyond_the_cutoff():
    """the kernels' own fp32 |r| never exceeds r_c; in fp64 the generic direction at r == r_c is over it by less than one fp32
    rounding -- an edge a builder accepted in fp64 and then rounded to fp32 components"""
    for vec, rc in ((lattice_edges(), RC), (radial_edges(), RC), (radial_edges(6.0, 5.5), 6.0), (sized_edges(257), RC)):
        assert (length_fp32(vec) <= np.float32(rc)).all()
        assert (_norm64(vec) <= rc * (1 + 2.0 ** -24)).all()
    assert length_fp32(radial_edges())[[26, 53]].tolist() == [5.0, 5.0]


def test_sizes_and_parameter_sets():
    assert SIZES == (1, 255, 256, 257)
    lat = lattice_edges()
    for n in SIZES:
        v = sized_edges(n)
        assert v.shape == (n, 3) and np.array_equal(v[:248], lat[:n]) and np.array_equal(v[248:], lat[:max(0, n - 248)])
    assert len(PARAMS) == 23 and len(set(PARAMS)) == 23 and len({p.id for p in PARAMS}) == 23
    base = [p for p in PARAMS if (p.n_basis, p.poly_p, p.rc) == (8, 6, RC)]
    assert {(p.lmax, p.normalize, p.kind) for p in base} == {(a, b, c) for a in range(4) for b in (0, 1) for c in (0, 1)}
    rest = [p for p in PARAMS if p not in base]
    assert all(p.lmax == 2 for p in rest)
    assert sorted((p.n_basis, p.poly_p, p.kind, p.rc, p.r_on) for p in rest) == sorted(
        [(1, 6, k, RC, R_ON) for k in (0, 1)] + [(16, 6, k, RC, R_ON) for k in (0, 1)] + [(8, 5, k, RC, R_ON) for k in (0, 1)]
        + [(8, 6, 1, 6.0, 5.5)])
    p = PARAMS[-1]
    assert p.coeffs().dtype == np.float32 and np.array_equal(p.coeffs(), np.array([n * np.pi / 6.0 for n in range(1, 9)], np.float32))


def test_edge_of_row_map_permutes_repeats_and_omits():
    m = edge_of_row_map(248)
    assert m.dtype == np.int32 and m.min() == 0 and m.max() < 248
    counts = np.bincount(m, minlength=248)
    assert (counts[1::2] == 0).all() and counts[0] == 6 and counts[246] == 3 and (counts[2:246:2] == 1).all()
    assert not np.array_equal(m[:124], np.arange(0, 248, 2))


def test_force_graph_has_every_kind_of_atom():
    fg = force_graph()
    seg, n, E = fg['seg_ptr'], fg['n'], fg['E']
    assert tuple(seg.tolist()) == FORCE_SEG and n == 300 and len(seg) - 1 == 7
    assert seg[1] == seg[2] and seg[3] - seg[2] == 1                                  # an empty segment, a one-atom system
    deg_in, deg_out = np.diff(fg['row_ptr']), np.diff(fg['col_ptr'])
    assert deg_in.sum() == E == deg_out.sum() and deg_in[40] == 0 == deg_out[40]      # ... which has no edges
    assert deg_in.min() == 0 and deg_in.max() == 70 and 69 in deg_in
    assert ((deg_in > 0) & (deg_out == 0)).any() and ((deg_in == 0) & (deg_out > 0)).any() and ((deg_in == 0) & (deg_out == 0)).any()
    center, src = fg['center'], fg['src']
    assert np.array_equal(center, np.repeat(np.arange(n), deg_in)) and (np.diff(center) >= 0).all()
    sys_of = lambda a: np.searchsorted(seg, a, side='right') - 1  # noqa: E731
    assert np.array_equal(sys_of(center), sys_of(src))                                # no edge leaves its system
    assert np.array_equal(np.sort(fg['eperm']), np.arange(E)) and (np.diff(src[fg['eperm']]) >= 0).all()
    assert np.array_equal(np.bincount(src, minlength=n), deg_out)
    # the six Voigt slots differ by more than a factor of 10 from one another, per system, and none of the per-system sums cancels
    F, va = force_reference64(fg)
    from oracle.model import force_virial_from_edge
    o = force_virial_from_edge(torch.as_tensor(fg['g']).double(), torch.as_tensor(fg['rij']).double(),
                               torch.as_tensor(np.stack([center, src])), n)
    assert np.array_equal(o['forces'].numpy(), F) and np.array_equal(o['atomic_virial'].numpy(), va)
    for b in range(7):
        rows = va[seg[b]:seg[b + 1]]
        if seg[b + 1] - seg[b] < 2:
            assert not rows.any()
            continue
        tot = np.abs(rows.sum(0))      # (a 1e-12 relative bar on an fp64 sum needs |sum| well above 1e-4 sum|terms|)
        assert (tot >= 1e-3 * np.abs(rows).sum(0)).all(), (b, tot / np.abs(rows).sum(0))
        mag = np.sort(np.abs(rows).max(0))
        assert (mag[1:] / mag[:-1] > 10).all(), (b, mag)
    assert (np.abs(va.sum(0)) >= 1e-3 * np.abs(va).sum(0)).all()                     # ... nor does the total
    assert np.isfinite(F).all() and np.abs(F.sum(0)).max() <= 1e-9 * np.abs(F).max()


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize('p', PARAMS, ids=lambda p: p.id)
def test_reference_is_finite_and_restatement_is_inside_the_asserted_bounds(p):
    for group in GROUPS:
        vec, ref, r32 = cached_reference(p, group)
        E = len(vec)
        assert E == (248 if group == 'lattice' else 54)
        assert ref['emb'].shape == (E, p.n_basis) == ref['demb'].shape and ref['sh'].shape == (E, p.nsh)
        assert ref['dsh'].shape == (E, p.nsh, 3)
        assert all(np.isfinite(ref[k]).all() for k in ref) and all(np.isfinite(r32[k]).all() for k in r32)
        assert all(r32[k].dtype == np.float32 for k in r32)
        err = {k: np.abs(r32[k].astype(np.float64) - ref[k]).max() for k in r32}
        print(f'{p.id} {group}: restatement vs fp64 ' + ', '.join(f'{k} {v:.2e} (max {np.abs(ref[k]).max():.3g})' for k, v in err.items()))
        assert err['emb'] < 2e-6
        assert err['sh'] < 5e-6 * max(1.0, np.abs(ref['sh']).max())
        # the reference vanishes at the cutoff with the envelope (the last radial edge of each direction: r == r_c in fp32)
        if group == 'radial':
            assert np.abs(ref['emb'][[26, 53]]).max() < 1e-12 and np.abs(r32['emb'][[26, 53]]).max() < 2e-6
        if p.lmax == 0:
            assert (ref['sh'] == 1).all() and not ref['dsh'].any()


def test_analytic_tangent_equals_autograd():
    """d emb / d|r| of edge_ref.reference64 (autograd) against the closed form tests/test_tangent_cpu.py pins the tangent kernels to"""
    from test_tangent_cpu import embedding_and_tangent
    for p in PARAMS:
        for group in GROUPS:
            _, ref, _ = cached_reference(p, group)
            emb, demb = embedding_and_tangent(torch.as_tensor(ref['r']), torch.as_tensor(p.coeffs()).double(), p.rc,
                                              'XPLOR' if p.kind else 'poly_cut', p.poly_p, p.r_on)
            assert np.abs(emb.numpy() - ref['emb']).max() <= 1e-13 and np.abs(demb.numpy() - ref['demb']).max() <= 1e-12


@pytest.mark.parametrize('normalize', [0, 1])
def test_oracle_harmonics_equal_the_engine_polynomials_in_fp64(normalize):
    """two derivations of the same polynomials -- the oracle's tensor recursion and sevennet_amd.irreps.sh_polynomials, from which
    the kernels' sh_eval / sh_grad / sh_jac are generated -- on every lattice vector, lmax 0..3"""
    from oracle.e3 import spherical_harmonics
    from sevennet_amd.irreps import sh_polynomials
    v = lattice_edges().astype(np.float64)
    u = v / np.linalg.norm(v, axis=1, keepdims=True) if normalize else v
    for lmax in range(4):
        want = spherical_harmonics(lmax, torch.as_tensor(v), bool(normalize)).numpy()
        cols = [sum(c * u[:, 0] ** k[0] * u[:, 1] ** k[1] * u[:, 2] ** k[2] for k, c in poly.items())
                for polys_l in sh_polynomials(lmax) for poly in polys_l]
        got = np.stack([np.broadcast_to(c, (len(v),)) for c in cols], 1)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
