"""CPU: the conditions the all-element D3 tests (test_d3_elements_gpu.py) rest on -- the two 94-element cells of d3_elements.py
are what they claim to be, the dimer closed form is the oracle's D3, and the oracle itself is permutation-covariant and has
forces that are the derivative of its energy where the C6 average is well defined."""
import numpy as np
import pytest

import d3_elements as E

CELL_PBC = sorted({(c, p) for c, p, _, _ in E.CASES})   # every (cell, pbc) the GPU cases use


def test_element_classes_are_the_blobs():
    mxc = E.tables()['mxc']
    assert tuple(z for z in range(1, 95) if mxc[z] == 1) == E.ONE_REF
    assert tuple(z for z in range(1, 95) if mxc[z] == 5) == E.FIVE_REF


@pytest.mark.parametrize('name', ['DILUTE', 'DENSE'])
def test_cells_hold_every_element_once_and_every_pair_interacts(name):
    Z, pos, cell = E.named_cell(name)
    assert sorted(Z.tolist()) == list(range(1, 95)) and pos.shape == (94, 3)
    assert not np.array_equal(Z, np.sort(Z)) and not np.array_equal(Z, np.sort(Z)[::-1])   # shuffled: first-seen order is neither
    frac = pos @ np.linalg.inv(cell)
    assert frac.min() > 0.03 and frac.max() < 0.97      # inside the cell with room for the finite-difference steps
    for pbc in sorted({p for c, p in CELL_PBC if c == name}):
        seen = {(i, j) for i, j, *_ in E.pairs_inside(pos, cell, pbc, E.VDW_CUT) if i != j}
        assert len(seen) == 94 * 93, (name, pbc, len(seen))


def test_dilute_is_far_from_the_fallback_and_dense_is_deep_in_it():
    """DILUTE: every pair's den is above 1e-60, so C6 is the smooth Gaussian average and the forces are true derivatives.
    DENSE: at least 1 000 ordered pairs on either side of den = 1e-99 for every pbc used, none within 1 % of it (fp64 rounding
    cannot send the oracle and the kernel down different branches), and the fallback meets elements with one and with five
    reference coordination numbers."""
    mxc = E.tables()['mxc']
    for name, pbc in CELL_PBC:
        Z, pos, cell = E.named_cell(name)
        cn = E.coordination_numbers(Z, pos, cell, pbc)
        if pbc == E.TTT:   # (the two oracle evaluations the tests below need anyway)
            assert np.abs(cn - E.oracle_result(name, pbc)['cn']).max() <= 1e-12 * cn.max()
        den = E.c6_den(Z, cn)
        fb = den <= 1e-99
        print(f'{name} pbc {pbc}: CN {cn.min():.3f} .. {cn.max():.2f}, fallback {fb.sum()}, normal {(~fb).sum()}, smallest den '
              f'{den.min():.2e}, closest |den / 1e-99 - 1| {np.abs(den / 1e-99 - 1).min():.3f}')
        if name == 'DILUTE':
            assert den.min() > 1e-60, (pbc, den.min())
            continue
        assert fb.sum() >= 1000 and (~fb).sum() >= 1000, (pbc, fb.sum(), (~fb).sum())
        assert np.abs(den / 1e-99 - 1).min() > 0.01, (pbc, np.abs(den / 1e-99 - 1).min())
        for k in (1, 5):
            has = mxc[Z] == k
            assert (fb & (has[:, None] | has[None, :])).any(), (pbc, k)


def test_every_elements_last_reference_carries_weight_somewhere():
    """what lets the GPU tests notice mxc[Z] one too small, for every Z: in at least one case (a cell of CELL_PBC, or a dimer, whose
    CN runs over 0 .. 1) the element's CN is such that its LAST reference is the nearest one (the fallback picks it) or weighs at least
    exp(-4 * 3.5) = 8e-7 of the nearest (the Gaussian average then moves by ~1e-7, a hundred times the 1e-9 bars).  With seed 10
    for DENSE this failed for cobalt alone (CN 4.5 against references 0, 1.7, 2.9, 7.8) -- and dropping cobalt's last reference
    then changed no energy or force of any case by more than 3e-14."""
    T = E.tables()
    mxc = T['mxc']

    def carries(z, cn):
        d = (T['cna'][z, z, :mxc[z], 0] - cn) ** 2
        return d[mxc[z] - 1] - d.min() < 3.5

    seen = {z for z in range(1, 95) if any(carries(z, cn) for cn in (0.05, 0.5, 0.95))}
    for name, pbc in CELL_PBC:
        Z, pos, cell = E.named_cell(name)
        seen |= {int(z) for z, cn in zip(Z, E.coordination_numbers(Z, pos, cell, pbc)) if carries(z, cn)}
    assert seen == set(range(1, 95)), sorted(set(range(1, 95)) - seen)


@pytest.fixture(scope='module')
def dimers():
    """the oracle on dimer_sample(), both dampings: energy, the force on the second atom along the axis, both CNs"""
    from oracle.d3 import d3
    zi, zj, r = E.dimer_sample()
    out = {}
    for damp in ('damp_bj', 'damp_zero'):
        rows = []
        for a, b, x in zip(zi, zj, r):
            o = d3([a, b], [[20.0, 20.0, 20.0], [20.0 + x, 20.0, 20.0]], np.eye(3) * 40.0, [False] * 3, damping=damp,
                   vdw_cutoff=E.VDW_CUT, cn_cutoff=E.CN_CUT)
            assert np.abs(o['forces'][:, 1:]).max() == 0.0 and abs(o['forces'][:, 0].sum()) < 1e-15
            rows.append((o['energy'], o['forces'][1, 0], o['cn'][0], o['cn'][1]))
        out[damp] = np.array(rows).T
    return out


@pytest.mark.parametrize('damp', ['damp_bj', 'damp_zero'])
def test_dimer_closed_form_is_the_oracle(dimers, damp):
    zi, zj, r = E.dimer_sample()
    assert len(zi) >= 40 and set(E.ONE_REF + E.FIVE_REF) <= set(zi.tolist()) | set(zj.tolist())
    e, fx, cn_a, cn_b = dimers[damp]
    ce, ca, cb = E.dimer_closed_form(zi, zj, r, damp, 'pbe')
    err_e, err_cn = np.abs(ce / e - 1).max(), max(np.abs(ca / cn_a - 1).max(), np.abs(cb / cn_b - 1).max())
    print(f'{damp}: closed form against the oracle, energy {err_e:.2e}, CN {err_cn:.2e} relative')
    assert err_e < 1e-12 and err_cn < 1e-12
    # the force: what test_d3_elements_gpu.py asks of all 4 465 pairs, here against the oracle's autograd force
    f = E.dimer_force(zi, zj, r, damp, 'pbe', E.DIMER_FD_STEP)
    defect = (np.abs(f - fx) / (np.abs(fx) + np.abs(e) / r)).max()
    print(f'{damp}: central difference of the closed form against the oracle force: {defect:.2e} of |F| + |E| / r')
    assert defect <= E.DIMER_FD_DEFECT


def test_oracle_is_permutation_covariant_on_dense():
    from oracle.d3 import d3
    Z, pos, cell = E.named_cell('DENSE')
    a = E.oracle_result('DENSE', E.TTT)
    p = np.argsort(Z)
    b = d3(Z[p], pos[p], cell, [True] * 3, vdw_cutoff=E.VDW_CUT, cn_cutoff=E.CN_CUT)
    assert np.abs(b['cn'] - a['cn'][p]).max() <= 1e-12 * np.abs(a['cn']).max()
    assert np.abs(b['forces'] - a['forces'][p]).max() <= 1e-12 * np.abs(a['forces']).max()
    assert np.abs(b['c6'] - a['c6'][np.ix_(p, p)]).max() <= 1e-12 * np.abs(a['c6']).max()
    assert abs(b['energy'] - a['energy']) <= 1e-12 * abs(a['energy'])


def test_the_fd_step_moves_no_pair_across_a_cutoff():
    Z, pos, cell = E.named_cell('DILUTE')
    d = E.FD_STEP * E.fd_direction()
    for cut in (E.VDW_CUT, E.CN_CUT):
        plus, minus = E.pairs_inside(pos + d, cell, E.TTT, cut), E.pairs_inside(pos - d, cell, E.TTT, cut)
        assert plus == minus and len(plus) > 10000


@pytest.mark.parametrize('damp', ['damp_bj', 'damp_zero'])
def test_oracle_forces_are_the_derivative_of_its_energy_on_dilute(damp):
    """with the pair sets fixed (above) there is no sharp-cutoff term: what is left is the truncation error of the step"""
    from oracle.d3 import d3
    Z, pos, cell = E.named_cell('DILUTE')
    d, h = E.fd_direction(), E.FD_STEP
    ev = lambda p: d3(Z, p, cell, [True] * 3, damping=damp, vdw_cutoff=E.VDW_CUT, cn_cutoff=E.CN_CUT)['energy']   # noqa: E731
    rhs = -(E.oracle_result('DILUTE', E.TTT, damp)['forces'] * d).sum()
    lhs = (ev(pos + h * d) - ev(pos - h * d)) / (2 * h)
    defect = abs(lhs - rhs) / abs(rhs)
    print(f'{damp}: dE/dh {lhs:.12g}, -sum F.d {rhs:.12g}, defect {defect:.2e} relative')
    assert abs(rhs) > 1.0 and defect <= E.FD_DEFECT
