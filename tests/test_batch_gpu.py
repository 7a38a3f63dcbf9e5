"""GPU: batched evaluation -- the batched neighbor list, the per-system reductions and the public batch surfaces against the
single-structure path and the fp64 oracle, on one heterogeneous batch: bulk Si (64 atoms), a rattled triclinic two-species
cell, a two-atom primitive cell thinner than the cutoff, a slab with one open axis, a molecule without a cell and one
isolated atom."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import oracle_model

pytestmark = pytest.mark.gpu

Z = [14, 8, 6, 1]   # atomic numbers of species 0..3


def _systems(n_species):
    from sevennet_amd.neighbor import diamond_cubic
    rng = np.random.default_rng(7)
    out = []
    pos, cell = diamond_cubic(5.431, (2, 2, 2), 0.05, 0)                                   # bulk Si, 64 atoms
    out.append((np.zeros(64, np.int64), pos, cell, [True] * 3))
    tri = np.array([[5.4, 0.0, 0.0], [1.0, 5.2, 0.0], [0.5, 0.8, 5.6]])                    # rattled triclinic, two species
    p0, _ = diamond_cubic(1.0, (1, 1, 1))
    out.append((rng.integers(0, 2, 8) % n_species, p0 @ tri + rng.normal(0, 0.08, (8, 3)), tri, [True] * 3))
    a = 5.431                                                                               # primitive cell thinner than rc
    prim = 0.5 * a * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    out.append((np.array([0, 1]) % n_species, np.array([[0.0, 0.0, 0.0], [a / 4, a / 4, a / 4 + 0.03]]), prim, [True] * 3))
    ps, cs = diamond_cubic(5.431, (2, 2, 1), 0.04, 2)                                       # slab: z open, zero cell row
    cs = cs.copy()
    cs[2] = 0.0
    out.append((rng.integers(0, n_species, len(ps)), ps + np.array([0, 0, 3.0]), cs, [True, True, False]))
    mol = np.array([[0.0, 0.0, 0.0], [1.1, 0.0, 0.0], [-0.4, 1.0, 0.0], [0.2, -0.5, 1.0], [2.3, 0.4, -0.6]])
    out.append((np.array([0, 1, 1, 0, 1]) % n_species, mol, np.zeros((3, 3)), [False] * 3))   # molecule, zero cell
    out.append((np.array([n_species - 1]), np.array([[0.3, -0.2, 0.1]]), np.zeros((3, 3)), [False] * 3))   # isolated atom
    return out


def _configs():
    from sevennet_amd.shapes import mini_sevennet_0_config, unit_test_config
    return {'mini_7net0': mini_sevennet_0_config(),   # layer 0 fused
            'unit_fctp': unit_test_config(),           # per-species (FCTP) self-connection
            'unit_species_rescale': unit_test_config(shift=[-1.0, -2.5, 0.5, -4.0], scale=[1.5, 0.5, 2.0, 1.0])}


def _calc(cfg, seed=0, **kw):
    from sevennet_amd.calculator import SevenNetCalculator
    from sevennet_amd.synthetic import random_state_dict
    ns = cfg['_number_of_species']
    cfg = dict(cfg, _type_map={Z[s]: s for s in range(ns)})
    sd = random_state_dict(cfg, seed=seed)
    return SevenNetCalculator((cfg, sd), file_type='model_instance', device='cuda:0', **kw), cfg, sd


def _batch(calc, systems, **kw):
    from sevennet_amd.batch import build_batch_graph
    eng = calc.model
    return build_batch_graph([s[0] for s in systems], [s[1] for s in systems], np.stack([s[2] for s in systems]),
                             np.array([s[3] for s in systems]), calc.cutoff, eng.spec.num_species, device='cuda:0',
                             species_rows=eng.needs_species_rows, **kw)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


@pytest.mark.parametrize('max_atoms', [2048, 32])
def test_batched_edges_equal_the_host_list(max_atoms):
    """per system, the batched edge set (center, src, shift) == neighbor.neighbor_list as a sorted set, edge_vec to 1e-6 A;
    max_atoms = 32 sends the 64-atom cell through the cell list and splices it in (concat_graphs)"""
    from sevennet_amd.batch import build_batch_graph
    from sevennet_amd.neighbor import neighbor_list
    rc = 5.0
    systems = _systems(2)
    g = build_batch_graph([s[0] for s in systems], [s[1] for s in systems], np.stack([s[2] for s in systems]),
                          np.array([s[3] for s in systems]), rc, 2, device='cuda:0', with_shifts=True, max_atoms=max_atoms)
    sp = g.seg_ptr_host
    assert sp.tolist() == np.concatenate([[0], np.cumsum([len(s[0]) for s in systems])]).tolist()
    rp, cen, src = _host(g.row_ptr), _host(g.center), _host(g.src)
    sh, ev = _host(g.shifts), _host(g.edge_vec)
    assert (np.repeat(np.arange(g.n_local), np.diff(rp)) == cen).all()
    for b, (types, pos, cell, pbc) in enumerate(systems):
        ei, evh, shh = neighbor_list(pos, cell, pbc, rc)
        a0, e0, e1 = sp[b], rp[sp[b]], rp[sp[b + 1]]
        got = np.concatenate([cen[e0:e1, None] - a0, src[e0:e1, None] - a0, sh[e0:e1]], 1)
        want = np.concatenate([ei.T, shh], 1)
        assert len(got) == len(want), (b, len(got), len(want))
        og, ow = np.lexsort(got.T[::-1]), np.lexsort(want.T[::-1])
        assert np.array_equal(got[og], want[ow]), b
        assert np.abs(ev[e0:e1][og] - evh[ow]).max(initial=0.0) < 1e-6, b
        assert np.array_equal(_host(g.types)[a0:sp[b + 1]], types)
    assert rp[sp[-1]] == rp[sp[-2]]   # the isolated atom: no edges


@pytest.mark.parametrize('name', ['mini_7net0', 'unit_fctp', 'unit_species_rescale'])
def test_batch_equals_single_structure_calls(name):
    calc, cfg, sd = _calc(_configs()[name], compute_atomic_virial=True)
    systems = _systems(cfg['_number_of_species'])
    g = _batch(calc, systems)
    out = calc.model.compute(g, want_atomic_virial=True)
    e_sys, vir_sys = _host(out['energy_per_system']), _host(out['virial_per_system'])
    forces, e_atom = _host(out['forces']), _host(out['atomic_energy'])
    assert e_sys.dtype == np.float64 and e_sys.shape == (len(systems),) and vir_sys.shape == (len(systems), 6)
    assert abs(e_sys.sum() - float(_host(out['energy'])[0])) <= 1e-12 * max(1.0, np.abs(e_sys).sum())
    sp = g.seg_ptr_host
    many = calc.compute_many([np.array(Z)[s[0]] for s in systems], [s[1] for s in systems], np.stack([s[2] for s in systems]),
                             np.array([s[3] for s in systems]))
    for b, (types, pos, cell, pbc) in enumerate(systems):
        one = calc.compute(np.array(Z)[types], pos, cell, pbc)
        a0, a1 = sp[b], sp[b + 1]
        assert abs(e_sys[b] - one['energy']) <= 1e-6 * abs(one['energy']) + 1e-6, (b, e_sys[b], one['energy'])
        f_tol = 2e-5 * max(1.0, np.abs(one['forces']).max())
        assert np.abs(forces[a0:a1] - one['forces']).max() <= f_tol, b
        assert np.abs(e_atom[a0:a1] - one['energies']).max() <= 1e-6 * max(1.0, np.abs(one['energies']).max()), b
        vol = abs(np.linalg.det(cell))
        if vol > 0:
            vir_one = -one['stress'][[0, 1, 2, 5, 3, 4]] * vol   # back to the engine's xx,yy,zz,xy,yz,zx
            assert np.abs(vir_sys[b] - vir_one).max() <= 1e-5 * max(1e-3, np.abs(vir_one).max()), b
        else:
            assert np.isnan(many[b]['stress']).all() and np.isnan(one['stress']).all()
        # compute_many: the same dict as compute, from the same batched evaluation
        m = many[b]
        assert set(m) == set(one)
        assert m['energy'] == m['free_energy'] == e_sys[b] and m['num_edges'] == one['num_edges']
        assert np.array_equal(m['forces'], forces[a0:a1]) and m['stresses'].shape == (a1 - a0, 6)
        assert np.allclose(m['stress'], one['stress'], rtol=0, atol=1e-5 * max(1e-3, np.nanmax(np.abs(one['stress']), initial=0)),
                           equal_nan=True)


def test_batch_against_the_fp64_oracle():
    calc, cfg, sd = _calc(_configs()['mini_7net0'])
    from sevennet_amd.neighbor import neighbor_list
    systems = _systems(cfg['_number_of_species'])
    res = calc.compute_many([np.array(Z)[s[0]] for s in systems], [s[1] for s in systems], np.stack([s[2] for s in systems]),
                            np.array([s[3] for s in systems]))
    orc = oracle_model(cfg, sd)
    for b, (types, pos, cell, pbc) in enumerate(systems):
        ei, ev, _ = neighbor_list(pos, cell, pbc, calc.cutoff)
        ref = orc.forward(types, ei, ev)
        assert abs(res[b]['energy'] - float(ref['energy'])) <= 1e-5 * abs(float(ref['energy'])) + 1e-5, b
        assert np.abs(res[b]['forces'] - ref['forces'].numpy()).max() < 1e-4, b


def test_isolated_atoms_on_a_fused_shape():
    """one atom per species, no edges at all (per-element reference energies): the fused layer-0 radial MLP gets E = 0"""
    calc, cfg, sd = _calc(_configs()['mini_7net0'])
    ns = cfg['_number_of_species']
    res = calc.compute_many([[Z[s]] for s in range(ns)], [np.zeros((1, 3))] * ns, np.zeros((ns, 3, 3)), [False] * 3)
    orc = oracle_model(cfg, sd)
    for s in range(ns):
        ref = orc.forward(np.array([s]), np.zeros((2, 0), np.int64), np.zeros((0, 3)))
        assert abs(res[s]['energy'] - float(ref['energy'])) <= 1e-6 * abs(float(ref['energy'])) + 1e-6
        assert np.array_equal(res[s]['forces'], np.zeros((1, 3))) and res[s]['num_edges'] == 0


def test_deterministic_and_order_preserving():
    calc, cfg, sd = _calc(_configs()['unit_species_rescale'])
    systems = _systems(cfg['_number_of_species'])
    outs = []
    for _ in range(2):
        out = calc.model.compute(_batch(calc, systems))
        outs.append({k: _host(out[k]).copy() for k in ('energy_per_system', 'virial_per_system', 'forces', 'energy')})
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    rev = calc.model.compute(_batch(calc, systems[::-1]))
    e_r, v_r, f_r = _host(rev['energy_per_system']), _host(rev['virial_per_system']), _host(rev['forces'])
    e, v, f = outs[0]['energy_per_system'], outs[0]['virial_per_system'], outs[0]['forces']
    assert np.allclose(e_r[::-1], e, rtol=1e-6, atol=1e-6)
    assert np.allclose(v_r[::-1], v, rtol=0, atol=1e-5 * np.abs(v).max())
    n = [len(s[0]) for s in systems]
    blocks = np.split(f, np.cumsum(n)[:-1])
    assert np.allclose(f_r, np.concatenate(blocks[::-1]), rtol=0, atol=2e-5 * max(1.0, np.abs(f).max()))


def test_torchsim_model_forward_matches_engine():
    from sevennet_amd.torchsim import SevenNetModel
    cfg0 = _configs()['mini_7net0']
    calc, cfg, sd = _calc(cfg0)
    systems = _systems(cfg['_number_of_species'])
    model = SevenNetModel((cfg, sd), device='cuda:0')
    dev = torch.device('cuda:0')
    n = [len(s[0]) for s in systems]
    state = SimpleNamespace(positions=torch.as_tensor(np.concatenate([s[1] for s in systems]), device=dev),
                            row_vector_cell=torch.as_tensor(np.stack([s[2] for s in systems]), device=dev),
                            pbc=torch.as_tensor(np.array([s[3] for s in systems]), device=dev),
                            atomic_numbers=torch.as_tensor(np.array(Z)[np.concatenate([s[0] for s in systems])], device=dev),
                            system_idx=torch.repeat_interleave(torch.arange(len(n), device=dev), torch.as_tensor(n, device=dev)))
    res = model.forward(state)
    assert res['energy'].shape == (len(n),) and res['forces'].shape == (sum(n), 3) and res['stress'].shape == (len(n), 3, 3)
    assert res['energy'].device == dev
    out = calc.model.compute(_batch(calc, systems))
    assert np.allclose(_host(res['energy']), _host(out['energy_per_system']), rtol=1e-6, atol=1e-5)
    assert np.allclose(_host(res['forces']), _host(out['forces']), rtol=0, atol=1e-6)
    many = calc.compute_many([np.array(Z)[s[0]] for s in systems], [s[1] for s in systems], np.stack([s[2] for s in systems]),
                             np.array([s[3] for s in systems]))
    from sevennet_amd.batch import voigt_to_3x3
    for b in range(len(n)):
        if abs(np.linalg.det(systems[b][2])) > 0:   # torch_sim's stress = the calculator's Voigt stress as a 3x3 tensor
            want = voigt_to_3x3(many[b]['stress'])
            assert np.allclose(_host(res['stress'][b]), want, rtol=1e-5, atol=1e-6 * max(1.0, np.abs(want).max())), b
