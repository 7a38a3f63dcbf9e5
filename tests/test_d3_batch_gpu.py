"""GPU: batched D3 dispersion (snet_d3_compute_batch through D3Engine / D3Calculator / SevenNetD3Calculator.compute_many)
on one heterogeneous batch -- the NaCl primitive cell, H2O without a cell, the 9-atom triclinic mixed cell (fully periodic and
with one open axis), a rattled 64-atom Si cell and one isolated atom: every system equals its own single call bit for bit,
and the fp64 oracle."""
import numpy as np
import pytest

from test_d3_cpu import H2O_POS, H2O_REF, NACL, NACL_REF, RTOL

pytestmark = pytest.mark.gpu

CUT = (1600.0, 900.0)   # reduced cutoffs (bohr^2) of test_d3_hip_vs_oracle


def _systems():
    from sevennet_amd.neighbor import diamond_cubic
    rng = np.random.default_rng(3)
    tri = np.array([[7.0, 0.4, 0.0], [0.3, 6.5, 0.5], [0.2, 0.6, 8.0]])
    tri_pos = rng.uniform(-0.3, 1.2, (9, 3)) @ tri
    tri_z = [6, 8, 1, 14, 8, 22, 1, 1, 79]
    si_pos, si_cell = diamond_cubic(5.431, (2, 2, 2), 0.05, 0)
    return [
        (NACL['numbers'], np.array(NACL['positions']), np.array(NACL['cell']), NACL['pbc']),   # 0: thin primitive cell
        ([8, 1, 1], H2O_POS, np.zeros((3, 3)), [False] * 3),                                  # 1: molecule, zero cell
        (tri_z, tri_pos, tri, [True] * 3),                                                    # 2: triclinic, periodic
        (tri_z, tri_pos, tri, [True, True, False]),                                           # 3: one open axis
        ([14] * len(si_pos), si_pos, si_cell, [True] * 3),                                    # 4: 64 rattled Si
        ([6], np.array([[0.3, -0.2, 0.1]]), np.zeros((3, 3)), [False] * 3),                   # 5: isolated atom
    ]


def _many(eng, systems):
    return eng.compute_many([s[0] for s in systems], [s[1] for s in systems], np.array([s[2] for s in systems], float),
                            np.array([s[3] for s in systems]))


def _assert_equal(a, b, what=''):
    assert a['energy'] == b['energy'], what
    for k in ('forces', 'stress', 'cn'):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


_ENGINES = {}


def _engine(damp, func, rthr, cnthr):
    from sevennet_amd.d3 import D3Engine
    key = (damp, func, rthr, cnthr)
    if key not in _ENGINES:
        _ENGINES[key] = D3Engine(damp, func, rthr, cnthr)
    return _ENGINES[key]


@pytest.mark.parametrize('damp,cut,subset', [('damp_bj', CUT, None), ('damp_zero', CUT, None),
                                             ('damp_bj', (9000.0, 1600.0), [0, 1, 3, 5])])
def test_batch_equals_single_calls_bitwise(damp, cut, subset):
    eng = _engine(damp, 'pbe', *cut)
    systems = _systems()
    if subset is not None:
        systems = [systems[i] for i in subset]
    many = _many(eng, systems)
    assert len(many) == len(systems)
    for b, s in enumerate(systems):
        _assert_equal(many[b], eng.compute(*s), f'system {b}')
    if subset is not None:   # default cutoffs: the reference's known answers from inside the batch
        nacl, h2o = many[0], many[1]
        assert abs(nacl['energy'] - NACL_REF['energy']) < RTOL * abs(NACL_REF['energy'])
        assert np.abs(nacl['forces'] - np.array(NACL_REF['forces'])).max() < RTOL * np.abs(NACL_REF['forces']).max()
        s = nacl['stress']
        voigt = np.array([s[0, 0], s[1, 1], s[2, 2], s[1, 2], s[0, 2], s[0, 1]])
        assert np.abs(voigt - np.array(NACL_REF['stress'])).max() < RTOL * np.abs(NACL_REF['stress']).max()
        assert abs(h2o['energy'] - H2O_REF['energy']) < 2e-6 * abs(H2O_REF['energy'])
        assert np.abs(h2o['forces'] - np.array(H2O_REF['forces'])).max() < RTOL * np.abs(H2O_REF['forces']).max()


@pytest.mark.parametrize('damp', ['damp_bj', 'damp_zero'])
def test_batch_against_the_fp64_oracle(damp):
    from oracle.d3 import d3
    from sevennet_amd.d3 import molecule_box
    systems = _systems()
    many = _many(_engine(damp, 'pbe', *CUT), systems)
    for b, (z, pos, cell, pbc) in enumerate(systems):
        if len(z) == 1:   # the isolated atom: its box is wider than both cutoffs, so nothing at all
            out = many[b]
            assert out['energy'] == 0.0 and not out['forces'].any() and not out['stress'].any() and not out['cn'].any()
            continue
        cell, pbc = molecule_box(pos, cell, pbc, *CUT)
        ref = d3(z, pos, cell, pbc, damping=damp, functional='pbe', vdw_cutoff=CUT[0], cn_cutoff=CUT[1])
        out = many[b]
        assert np.abs(out['cn'] - ref['cn']).max() <= 1e-10 * max(1.0, np.abs(ref['cn']).max()), b
        assert abs(out['energy'] - ref['energy']) <= 1e-9 * abs(ref['energy']), b
        assert np.abs(out['forces'] - ref['forces']).max() <= 1e-9 * max(1e-12, np.abs(ref['forces']).max()), b
        assert np.abs(out['stress'] - ref['stress']).max() <= 1e-9 * np.abs(ref['stress']).max(), b


def test_deterministic_and_order_preserving():
    eng = _engine('damp_bj', 'pbe', *CUT)
    systems = _systems()
    a, b = _many(eng, systems), _many(eng, systems)
    r = _many(eng, systems[::-1])[::-1]
    for k in range(len(systems)):
        _assert_equal(a[k], b[k], f'repeat {k}')
        _assert_equal(a[k], r[k], f'reversed {k}')


def test_d3_term_is_one_compute_many_over_the_systems_asked_for():
    """the `extra` of the batched drivers: systems [2, 0] of the three small systems at perturbed positions (the molecule's box
    comes from those positions, not from the ones the term was built with)"""
    import torch
    from helpers import three_small_systems
    from sevennet_amd.d3 import D3Term
    eng = _engine('damp_bj', 'pbe', *CUT)
    systems = three_small_systems()
    z = [np.array([14, 8])[s[0]] for s in systems]
    term = D3Term(eng, np.concatenate(z), [len(s[0]) for s in systems], np.stack([s[2] for s in systems]),
                  np.array([s[3] for s in systems]))
    rng = np.random.default_rng(4)
    for ids in ([2, 0], [1]):
        moved = [systems[b][1] + rng.normal(0, 0.1, systems[b][1].shape) for b in ids]
        pos = torch.as_tensor(np.concatenate(moved)).to('cuda:0')
        seg_ptr = np.concatenate([[0], np.cumsum([len(m) for m in moved])])
        forces, energies = term(pos, seg_ptr, np.array(ids))
        want = eng.compute_many([z[b] for b in ids], moved, np.stack([systems[b][2] for b in ids]), np.array([systems[b][3] for b in ids]))
        assert forces.device == pos.device and energies.device == pos.device
        assert forces.dtype == torch.float64 and energies.dtype == torch.float64
        assert np.array_equal(forces.cpu().numpy(), np.concatenate([w['forces'] for w in want]))
        assert energies.cpu().numpy().tolist() == [w['energy'] for w in want]
        assert len(term.last) == len(ids)
        for got, w in zip(term.last, want):
            _assert_equal(got, w, f'systems {ids}')
    assert np.abs(term.last[0]['forces']).max() > 0   # the molecule: its box did not turn the term off


def test_a_large_cell_among_small_ones():
    """1 000 Si atoms (t_chunks = 1) beside cells of 1 .. 64 atoms (t_chunks > 1): each keeps its own traversal"""
    from sevennet_amd.neighbor import diamond_cubic
    eng = _engine('damp_bj', 'pbe', *CUT)
    pos, cell = diamond_cubic(5.431, (5, 5, 5), 0.03, 4)
    systems = _systems()
    systems = systems[:2] + [([14] * len(pos), pos, cell, [True] * 3)] + systems[4:]
    many = _many(eng, systems)
    for b, s in enumerate(systems):
        _assert_equal(many[b], eng.compute(*s), f'system {b}')


def test_d3_calculator_compute_many():
    from sevennet_amd.d3 import D3Calculator
    calc = D3Calculator(vdw_cutoff=CUT[0], cn_cutoff=CUT[1])
    systems = _systems()
    many = _many(calc, systems)
    for b, s in enumerate(systems):
        one = calc.compute(*s)
        assert set(many[b]) == set(one) and many[b]['stress'].shape == (6,)
        for k in one:
            assert np.array_equal(many[b][k], one[k]), (b, k)


class _Atoms:
    """the four getters compute_many reads from an ASE Atoms"""

    def __init__(self, z, pos, cell, pbc):
        self.z, self.pos, self.cell, self.pbc = z, pos, cell, pbc

    def get_atomic_numbers(self):
        return np.asarray(self.z)

    def get_positions(self):
        return np.asarray(self.pos, float)

    def get_cell(self):
        return np.asarray(self.cell, float)

    def get_pbc(self):
        return np.asarray(self.pbc, bool)


def test_sevennet_d3_calculator_compute_many():
    from sevennet_amd.d3 import SevenNetD3Calculator
    from sevennet_amd.shapes import mini_sevennet_0_config
    from sevennet_amd.synthetic import random_state_dict
    Z = [14, 8, 6, 1]
    cfg = mini_sevennet_0_config(len(Z))
    cfg['_type_map'] = {z: s for s, z in enumerate(Z)}
    calc = SevenNetD3Calculator((cfg, random_state_dict(cfg, seed=0)), file_type='model_instance', device='cuda:0',
                                vdw_cutoff=CUT[0], cn_cutoff=CUT[1])
    systems = _systems()
    rng = np.random.default_rng(11)   # elements the model knows
    systems[2] = (list(rng.choice(Z, 9)), systems[2][1], systems[2][2], systems[2][3])
    systems[3] = (systems[2][0], systems[3][1], systems[3][2], systems[3][3])
    systems = systems[1:]   # the NaCl cell holds elements the model does not know
    systems[-1] = ([1], systems[-1][1], systems[-1][2], systems[-1][3])
    many = _many(calc, systems)
    sn_calc, d3_calc = calc.calcs
    sn_many = _many(sn_calc, systems)
    for b, s in enumerate(systems):
        one = calc.compute(*s)
        m = many[b]
        assert set(m) == set(one), b
        d3_one = d3_calc.compute(*s)
        # the D3 share is the single call's, bit for bit
        for k in ('free_energy', 'energy', 'forces', 'stress'):
            assert np.array_equal(m[k], sn_many[b][k] + d3_one[k], equal_nan=True), (b, k)
        # the model share: the tolerances of test_batch_equals_single_structure_calls
        assert abs(m['energy'] - one['energy']) <= 1e-6 * abs(one['energy']) + 1e-6, b
        assert m['free_energy'] == m['energy'] and m['num_edges'] == one['num_edges']
        assert np.abs(m['forces'] - one['forces']).max() <= 2e-5 * max(1.0, np.abs(one['forces']).max()), b
        if abs(np.linalg.det(s[2])) > 0:
            assert np.allclose(m['stress'], one['stress'], rtol=0, atol=1e-5 * max(1e-3, np.abs(one['stress']).max())), b
        else:   # a zero cell: NaN model stress, as compute gives
            assert np.isnan(m['stress']).all() and np.isnan(one['stress']).all(), b
    via_atoms = calc.calculate_many([_Atoms(*s) for s in systems])
    for b in range(len(systems)):
        assert set(via_atoms[b]) == set(many[b])
        for k in many[b]:
            assert np.array_equal(via_atoms[b][k], many[b][k], equal_nan=True), (b, k)
    d3_atoms = d3_calc.calculate_many([_Atoms(*s) for s in systems])
    d3_many = _many(d3_calc, systems)
    for b in range(len(systems)):
        for k in d3_many[b]:
            assert np.array_equal(d3_atoms[b][k], d3_many[b][k]), (b, k)
