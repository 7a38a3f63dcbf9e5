"""GPU: the HIP D3 term (csrc/snet_d3.hip) over all 94 elements of its tables and through the nearest-reference fallback of
d3_c6 (den <= 1e-99, reference pair_d3_for_ase.cu:833-837), which no other D3 test reaches: nt = 94 dense types, every r0ab /
r2r4 / rcov / mxc entry and every element pair's reference grid.  The cells, the closed form and the bars come from
d3_elements.py; test_d3_elements_cpu.py establishes them against the fp64 oracle."""
import numpy as np
import pytest

import d3_elements as E
from test_d3_batch_gpu import _assert_equal, _engine
from test_d3_cpu import voigt

pytestmark = pytest.mark.gpu

ASC = lambda Z: np.argsort(Z)          # noqa: E731
DESC = lambda Z: np.argsort(Z)[::-1]   # noqa: E731


def engine(damp='damp_bj', func='pbe'):
    return _engine(damp, func, E.VDW_CUT, E.CN_CUT)


@pytest.fixture(scope='module')
def oracle():
    """oracle.d3.d3 per case, computed once (1 - 3 s each on the CPU) and shared by the tests of this file"""
    return E.oracle_result


def _worst(err, Z):
    i = int(np.argmax(np.asarray(err).reshape(len(Z), -1).max(1)))
    return f'worst atom {i} (Z = {int(Z[i])})'


# ------------------------------------------------------------------------------------------------ (a) against the oracle
@pytest.mark.parametrize('name,pbc,damp,func', E.CASES, ids=[f'{c}-{"".join("FT"[x] for x in p)}-{d}-{f}' for c, p, d, f in E.CASES])
def test_all_elements_against_the_oracle(oracle, name, pbc, damp, func):
    """94 atoms = 94 types.  DILUTE: every pair on the Gaussian branch; DENSE: thousands of ordered pairs on either branch
    (counts in test_d3_elements_cpu.py).  The bars of test_d3_hip_vs_oracle."""
    Z, pos, cell = E.named_cell(name)
    ref = oracle(name, pbc, damp, func)
    out = engine(damp, func).compute(Z, pos, cell, list(pbc))
    err = np.abs(out['cn'] - ref['cn'])
    print(f'cn {err.max():.2e} of {max(1.0, np.abs(ref["cn"]).max()):.2f}, energy {abs(out["energy"] / ref["energy"] - 1):.2e}, forces '
          f'{np.abs(out["forces"] - ref["forces"]).max() / np.abs(ref["forces"]).max():.2e}, stress '
          f'{np.abs(out["stress"] - ref["stress"]).max() / np.abs(ref["stress"]).max():.2e}, net force '
          f'{np.abs(out["forces"].sum(0)).max() / (len(Z) * np.abs(out["forces"]).max()):.2e}')
    assert err.max() < 1e-10 * max(1.0, np.abs(ref['cn']).max()), ('cn', err.max(), _worst(err, Z))
    assert abs(out['energy'] - ref['energy']) < 1e-9 * abs(ref['energy']), (out['energy'], ref['energy'])
    err = np.abs(out['forces'] - ref['forces'])
    assert err.max() < 1e-9 * np.abs(ref['forces']).max(), ('forces', err.max(), _worst(err, Z))
    assert np.abs(out['stress'] - ref['stress']).max() < 1e-9 * np.abs(ref['stress']).max()
    assert np.abs(out['forces'].sum(0)).max() < 1e-12 * len(Z) * np.abs(out['forces']).max()


# ------------------------------------------------------------------------------------------------ (b) every pair on its own
@pytest.mark.parametrize('damp', ['damp_bj', 'damp_zero'])
def test_every_element_pair_as_a_dimer(damp):
    """all 4 465 unordered element pairs as two-atom molecules in ONE compute_many (8 930 atoms, nt = 94) against the closed
    form: a swapped r0ab / r2r4 / rcov / mxc entry or grid slice is one term of 4 465 in the 94-atom cells, here it is a system."""
    zi, zj, r, u = E.all_pairs()
    B = len(zi)
    assert B == 4465
    pos = np.empty((B, 2, 3))
    pos[:, 0], pos[:, 1] = 20.0 - 0.5 * r[:, None] * u, 20.0 + 0.5 * r[:, None] * u
    res = engine(damp).compute_many(np.stack([zi, zj], 1).reshape(-1), pos.reshape(-1, 3), np.tile(np.eye(3) * 40.0, (B, 1, 1)),
                                    np.zeros((B, 3), bool), n_atoms=np.full(B, 2))
    e = np.array([x['energy'] for x in res])
    cn = np.array([x['cn'] for x in res])
    f = np.array([x['forces'] for x in res])
    ce, ca, cb = E.dimer_closed_form(zi, zj, r, damp, 'pbe')
    err_e, err_cn = np.abs(e / ce - 1), np.abs(cn / np.stack([ca, cb], 1) - 1).max(1)
    scale = np.abs(E.dimer_force(zi, zj, r, damp, 'pbe', E.DIMER_FD_STEP)) + np.abs(ce) / r
    along = (f[:, 1] * u).sum(1)                     # the force on the second atom along the axis: -dE/dr
    err_sum = np.abs(f[:, 0] + f[:, 1]).max(1) / scale
    err_axis = np.abs(f[:, 1] - along[:, None] * u).max(1) / scale
    err_f = np.abs(along - E.dimer_force(zi, zj, r, damp, 'pbe', E.DIMER_FD_STEP)) / scale
    print(f'energy {err_e.max():.2e}, cn {err_cn.max():.2e}, f1 + f2 {err_sum.max():.2e}, off axis {err_axis.max():.2e}, '
          f'|F| against the central difference {err_f.max():.2e} (bar {10 * E.DIMER_FD_DEFECT:.1e})')
    at = lambda err: (float(err.max()), f'pair Z = {int(zi[np.argmax(err)])}, {int(zj[np.argmax(err)])} at {r[np.argmax(err)]:.3f} A')   # noqa: E731
    assert err_e.max() <= 1e-10, ('energy',) + at(err_e)
    assert err_cn.max() <= 1e-12, ('cn',) + at(err_cn)
    assert err_sum.max() <= 1e-12 and err_axis.max() <= 1e-12, (at(err_sum), at(err_axis))
    # (DIMER_FD_DEFECT is the same comparison against the oracle's forces on the CPU sample; x 10)
    assert err_f.max() <= 10 * E.DIMER_FD_DEFECT, ('force',) + at(err_f)


# ------------------------------------------------------------------------------------------------ (c) compaction
@pytest.mark.parametrize('damp', ['damp_bj', 'damp_zero'])
def test_the_order_of_first_appearance_does_not_matter(damp):
    """DENSE with its atoms Z-ascending, Z-descending and shuffled: three different dense type tables, one answer"""
    Z, pos, cell = E.named_cell('DENSE')
    eng = engine(damp)
    base = eng.compute(Z, pos, cell, [True] * 3)
    for order in (ASC, DESC):
        p = order(Z)
        out = eng.compute(Z[p], pos[p], cell, [True] * 3)
        want = dict(base, cn=base['cn'][p], forces=base['forces'][p])
        print(', '.join(f'{k} {np.abs(out[k] - want[k]).max() / np.abs(want[k]).max():.2e}' for k in ('cn', 'forces', 'energy', 'stress'))
              + ' (bar 1e-12)')
        for k in ('cn', 'forces'):
            err = np.abs(out[k] - base[k][p])
            assert err.max() <= 1e-12 * np.abs(base[k]).max(), (k, err.max(), _worst(err, Z[p]))
        assert abs(out['energy'] - base['energy']) <= 1e-12 * abs(base['energy'])
        assert np.abs(out['stress'] - base['stress']).max() <= 1e-12 * np.abs(base['stress']).max()


def _mixed_batch():
    """DENSE, nine of its atoms, DILUTE, eleven of its atoms of other elements than the nine: in the batch the small systems'
    types are scattered over the 94, alone they are 0 .. 8 and 0 .. 10"""
    Zd, pd, cd = E.named_cell('DENSE')
    Zl, pl, cl = E.named_cell('DILUTE')
    nine = np.arange(40, 49)
    eleven = np.nonzero(~np.isin(Zl, Zd[nine]))[0][5:16]
    assert len(set(Zd[nine]) | set(Zl[eleven])) == 20
    return [(Zd, pd, cd, E.TTT), (Zd[nine], pd[nine], cd, E.TTF), (Zl, pl, cl, E.TTT), (Zl[eleven], pl[eleven], cl, E.FFF)]


@pytest.mark.parametrize('damp', ['damp_bj', 'damp_zero'])
def test_a_mixed_batch_is_its_single_calls_and_the_device_path_bit_for_bit(damp):
    import torch
    from test_d3_device_gpu import _assert_is_the_host_path, _flat, _host_arrays, _volumes
    eng = engine(damp)
    systems = _mixed_batch()
    many = eng.compute_many([s[0] for s in systems], [s[1] for s in systems], np.array([s[2] for s in systems]),
                            np.array([s[3] for s in systems]))
    for b, s in enumerate(systems):
        _assert_equal(many[b], eng.compute(s[0], s[1], s[2], list(s[3])), f'system {b}')
        assert np.abs(many[b]['forces']).max() > 1e-4
    z, n_atoms, cells, pbcs = _flat(systems)
    plan = eng.plan(z, n_atoms, cells, pbcs)
    got = _host_arrays(eng.compute_device(plan, torch.as_tensor(np.concatenate([s[1] for s in systems])).cuda()))
    _assert_is_the_host_path(got, many, _volumes(systems), 'mixed batch')


# ------------------------------------------------------------------------------------------------ (d) derivatives
@pytest.mark.parametrize('damp', ['damp_bj', 'damp_zero'])
def test_forces_are_the_derivative_of_the_energy_with_all_elements(damp):
    """DILUTE, along the displacement that test_d3_elements_cpu.py shows to move no pair across either cutoff, so the bar is
    the oracle's own defect there (the truncation error of the step) x 10, plus 1e-9; then a rigid rotation.
    No such check on DENSE: in the fallback dC6/dCN is DEFINED as 0, as in the reference, while C6 jumps from reference point to
    reference point -- the forces there are not the derivative of the energy, in the reference or here."""
    Z, pos, cell = E.named_cell('DILUTE')
    eng = engine(damp)
    ev = lambda p, c: eng.compute(Z, p, c, [True] * 3)   # noqa: E731
    a = ev(pos, cell)
    d, h = E.fd_direction(), E.FD_STEP
    rhs = -(a['forces'] * d).sum()
    lhs = (ev(pos + h * d, cell)['energy'] - ev(pos - h * d, cell)['energy']) / (2 * h)
    print(f'dE/dh {lhs:.12g}, -sum F.d {rhs:.12g}: {abs(lhs - rhs) / abs(rhs):.2e} relative (bar {10 * E.FD_DEFECT + 1e-9:.1e})')
    assert abs(lhs - rhs) <= (10 * E.FD_DEFECT + 1e-9) * abs(rhs), (lhs, rhs)
    q, r = np.linalg.qr(np.random.default_rng(5).normal(size=(3, 3)))
    R = q * np.sign(np.diag(r))
    if np.linalg.det(R) < 0:
        R[:, 0] = -R[:, 0]
    b = ev(pos @ R.T, cell @ R.T)
    f, s = a['forces'], a['stress']
    print(f'rotation: energy {abs(b["energy"] / a["energy"] - 1):.2e} (bar 1e-10), forces {np.abs(b["forces"] - f @ R.T).max() / np.abs(f).max():.2e}, '
          f'stress {np.abs(b["stress"] - R @ s @ R.T).max() / np.abs(s).max():.2e} (bar 1e-9)')
    assert abs(b['energy'] - a['energy']) <= 1e-10 * abs(a['energy'])
    err = np.abs(b['forces'] - f @ R.T)
    assert err.max() <= 1e-9 * np.abs(f).max(), (err.max(), _worst(err, Z))
    assert np.abs(b['stress'] - R @ s @ R.T).max() <= 1e-9 * np.abs(s).max()


# ------------------------------------------------------------------------------------------------ (e) the reference's binding
@pytest.mark.parametrize('damp', ['damp_bj', 'damp_zero'])
def test_reference_binding_with_94_types(damp):
    """`pair_*` (csrc/snet_d3_ref.cpp) driven the reference's way: 94 one-based types in order of first appearance, the atomic
    numbers through pair_run_coeff, the cutoffs through pair_run_settings; in the rotated LAMMPS frame"""
    import ctypes
    from sevennet_amd import _lib
    from test_d3_gpu import _reference_calculate, _reference_stub
    lib = ctypes.CDLL(_lib.LIB_PATH)
    _reference_stub(lib)
    Z, pos, cell = E.named_cell('DENSE')
    ref = engine(damp).compute(Z, pos, cell, [True] * 3)
    e, f, s = _reference_calculate(lib, Z.tolist(), pos, cell, [True] * 3, damp.encode(), b'pbe', rthr=E.VDW_CUT, cnthr=E.CN_CUT)
    err = np.abs(f - ref['forces'])
    print(f'energy {abs(e / ref["energy"] - 1):.2e}, forces {err.max() / np.abs(ref["forces"]).max():.2e}, stress '
          f'{np.abs(s - voigt(ref["stress"])).max() / np.abs(ref["stress"]).max():.2e}')
    assert abs(e - ref['energy']) <= 1e-12 * abs(ref['energy'])
    assert err.max() <= 1e-12 * np.abs(ref['forces']).max(), (err.max(), _worst(err, Z))
    assert np.abs(s - voigt(ref['stress'])).max() <= 1e-12 * np.abs(ref['stress']).max()
