"""GPU: the first interaction layer's reverse pass from per-atom products (snet_layer0_conv_bwd, csrc/snet_layer0.hip) against
the fp64 evaluation of the direct per-edge formula (tests/test_layer0_moments_cpu.py) and against the fused per-edge kernel it
replaces, then the whole model: both hosts, the fp64 and fp32 oracles, the switch on and off."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_layer0_moments_cpu import HID, direct_reference, random_case
from test_ops_gpu import _lib, _p, _work_list

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CST_SILU = 1.6791767923989418
# degrees: no edge, 1, a full 16-edge tile, 17 (tile + 1), 33 (two tiles + 1), and a few ordinary rows
DEGREES = (0, 1, 16, 17, 33, 5, 12, 0, 28)


def _layer0_spec(model):
    from sevennet_amd.model_spec import build_model_spec, sevennet_0_config
    from sevennet_amd.shapes import mini_sevennet_0_config
    cfg = {'mini': mini_sevennet_0_config, 'sevennet_0': sevennet_0_config}[model]()
    return build_model_spec(cfg).layers[0].conv


def _run_ops(model, n_species, present, pairs, seed):
    """one random layer-0 reverse problem through snet_layer0_conv_bwd and through today's fused kernel -> (case, g_vec new, g_vec old)
    as fp64 numpy arrays"""
    L, lib = _lib()
    spec = _layer0_spec(model)
    mul, lmax = spec.irreps_x.dim, len(spec.paths) - 1
    c = random_case(mul=mul, lmax=lmax, n_species=n_species, present=present, degrees=DEGREES, n_ghost=3, seed=seed, dtype=np.float32)
    N, E, Q, wn, NT = c['N'], c['E'], (lmax + 1) ** 2, spec.weight_numel, len(c['types'])
    rng = np.random.default_rng(seed + 100)
    if pairs:   # several edges share one radial row, in scrambled order
        R = E // 2 + 3
        c['w_row'] = rng.integers(0, R, E).astype(np.int32)
        c['h2'], c['h2d'] = c['h2'][:R].copy(), c['h2d'][:R].copy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    vec = t(c['edge_vec'])
    P = L.EdgeParams(5.0, 8, 0, 6, 0.0, lmax, 1)
    cf = (C.c_float * 8)(*[(k + 1) * np.pi / 5.0 for k in range(8)])
    emb, sh, dsh = torch.empty(E, 8, device=DEV), torch.empty(E, Q, device=DEV), torch.empty(E, 3 * Q, device=DEV)
    L.check(lib.snet_edge_embed_fwd(C.byref(P), cf, _p(vec), E, _p(emb), _p(sh), _p(dsh), None))
    torch.cuda.synchronize()
    c['sh'], c['dsh'] = sh.cpu().numpy(), dsh.cpu().numpy()      # real harmonics and their Jacobian (fp32, as every kernel reads them)
    g_m = rng.normal(0, 1, (N, Q * mul)).astype(np.float32)
    h2, h2d, rp, src, types = t(c['h2']), t(c['h2d']), t(c['row_ptr']), t(c['src']), t(c['types'])
    wr = None if c['w_row'] is None else t(c['w_row'])
    gm = t(g_m)
    # ---- the moments path
    plan, lplan = C.c_void_p(), C.c_void_p()
    L.check(lib.snet_conv_plan_create(spec.tag.encode(), C.byref(plan)))
    pres = sorted(present)
    slot = np.zeros(n_species, np.int32)
    slot[pres] = np.arange(len(pres), dtype=np.int32)
    table_s = np.ascontiguousarray(c['table'][pres])
    L.check(lib.snet_layer0_plan_create(plan, C.c_void_p(c['W2'].ctypes.data), C.c_void_p(table_s.ctypes.data), c['scale'], len(pres),
                                        C.byref(lplan)), 'snet_layer0_plan_create')
    n_scr = int(lib.snet_layer0_scratch_size(lplan, N))
    assert n_scr == N * Q * len(pres) * HID
    scratch = torch.full((n_scr + 64,), float('nan'), device=DEV)
    gv_new = torch.zeros(E + 1, 3, device=DEV)
    sl = t(slot)
    L.check(lib.snet_layer0_conv_bwd(lplan, _p(gm), _p(h2), _p(h2d), _p(wr), _p(rp), _p(src), _p(types), _p(sl), _p(sh), _p(dsh), _p(vec), N,
                                     _p(scratch), _p(gv_new), None))
    torch.cuda.synchronize()
    assert torch.isnan(scratch[n_scr:]).all() and not torch.isnan(scratch[:n_scr]).any()      # Bm: every entry written, nothing beyond
    assert (gv_new[E] == 0).all() and not torch.isnan(gv_new).any()
    # no rows: nothing is launched, nothing is read
    L.check(lib.snet_layer0_conv_bwd(lplan, None, None, None, None, None, None, None, None, None, None, None, 0, None, None, None))
    # ---- today's fused kernel on the same inputs (engine default precision: fp16 terms, tangent mode)
    mlp, fplan = C.c_void_p(), C.c_void_p()
    W0, W1 = np.zeros((8, 64), np.float32), np.zeros((64, 64), np.float32)   # (the hidden layers are not run: h2 / h2' are inputs)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    L.check(lib.snet_radial_mlp_plan_create(8, 64, 64, wn, fp(W0), fp(W1), fp(c['W2']), 0, CST_SILU, 1, C.byref(mlp)))
    L.check(lib.snet_fused_plan_create(plan, mlp, 4, C.byref(fplan)))
    x = t(c['table'][c['types']])
    gv_old = torch.zeros(E, 3, device=DEV)
    tile_ptr, tile_node, n_tiles = _work_list(L, lib, fplan, rp, torch.from_numpy(c['row_ptr']), N, E, DEV)
    x_max, g_max = torch.empty(NT, device=DEV), torch.empty(N, device=DEV)
    L.check(lib.snet_row_absmax(_p(x), NT, mul, _p(x_max), None))
    L.check(lib.snet_row_absmax(_p(gm), N, Q * mul, _p(g_max), None))
    L.check(lib.snet_conv_bwd_fused_tangent(fplan, _p(x), _p(sh), _p(dsh), _p(h2), _p(h2d), _p(wr), _p(rp), _p(src), _p(tile_ptr),
                                            _p(tile_node), n_tiles.value, c['scale'], _p(gm), None, _p(vec), _p(gv_old), _p(x_max), _p(g_max),
                                            None))
    torch.cuda.synchronize()
    lib.snet_layer0_plan_destroy(lplan)
    lib.snet_fused_plan_destroy(fplan)
    lib.snet_conv_plan_destroy(plan)
    lib.snet_radial_mlp_plan_destroy(mlp)
    f64 = lambda a: a.double().cpu().numpy()  # noqa: E731
    c['g_m'] = g_m
    return c, f64(gv_new[:E]), f64(gv_old)


@pytest.mark.parametrize('model,n_species,present,pairs', [('mini', 1, (0,), False), ('mini', 2, (0, 1), True), ('mini', 3, (0, 2), True),
                                                           ('sevennet_0', 3, (0, 2), True), ('sevennet_0', 4, (0, 1, 2, 3), False)])
def test_reverse_entry_point_vs_fp64_and_the_fused_kernel(model, n_species, present, pairs):
    """g_vec against the fp64 direct formula; the project's fp32-class rule (tests/test_tangent_gpu.py): the new path's error is at most
    1.5 x the error of today's fused kernel on the same inputs.  Graph: rows of 0, 1, 16, 17 and 33 edges, ghost source rows,
    1 / 2 / 3 species with one slot unused (species 1 of three on no atom), radial rows shared by several edges."""
    c, new, old = _run_ops(model, n_species, present, pairs, seed=11 * n_species + len(present))
    ref = direct_reference(c, c['g_m'])
    e_new, e_old = np.abs(new - ref).max(), np.abs(old - ref).max()
    print(f'{model} S={len(present)}/{n_species} pairs={pairs} g_vec: max|ref| {np.abs(ref).max():.3g}, error vs fp64 fused {e_old:.3e} '
          f'per-atom {e_new:.3e}, ratio {e_new / e_old:.2f}')
    assert e_new <= 1.5 * e_old, (e_new, e_old)


def test_plan_refuses_shapes_outside_its_domain():
    from sevennet_amd.model_spec import build_model_spec, sevennet_0_config
    L, lib = _lib()
    layers = build_model_spec(sevennet_0_config()).layers
    W2, T = np.zeros((64, 4096), np.float32), np.zeros((4, 512), np.float32)
    for ls, ns in ((layers[1], 1), (layers[0], 0), (layers[0], 5)):     # non-scalar inputs; too few / too many species slots
        plan, lp = C.c_void_p(), C.c_void_p()
        L.check(lib.snet_conv_plan_create(ls.conv.tag.encode(), C.byref(plan)))
        assert lib.snet_layer0_plan_create(plan, C.c_void_p(W2.ctypes.data), C.c_void_p(T.ctypes.data), 1.0, ns, C.byref(lp)) != 0
        assert not lp.value and b'snet_layer0_plan_create' in lib.snet_last_error()
        lib.snet_conv_plan_destroy(plan)


@functools.lru_cache(maxsize=None)
def _smoke_cell():
    """the 64-atom rattled Si cell of smoke() with SevenNet-0's shape at max|F| = 8 eV/A, and both oracles' results (computed once)"""
    from oracle.model import OracleModel
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.neighbor import diamond_cubic, neighbor_list
    from sevennet_amd.synthetic import random_state_dict
    cfg = sevennet_0_config()
    sd = random_state_dict(cfg, seed=0)
    pos, cell = diamond_cubic(5.431, (2, 2, 2), 0.05, 0)
    ei, ev, _ = neighbor_list(pos, cell, [True] * 3, cfg['cutoff'])
    types = np.zeros(len(pos), np.int64)
    ref1 = OracleModel(cfg, sd, dtype=torch.float64).forward(types, ei, ev)
    sd = dict(sd)
    sd['rescale_atomic_energy.scale'] = (np.asarray(sd['rescale_atomic_energy.scale'], np.float64) * 8.0 / float(ref1['forces'].abs().max())).astype(np.float32)
    ref = OracleModel(cfg, sd, dtype=torch.float64).forward(types, ei, ev)
    r32 = OracleModel(cfg, sd, dtype=torch.float32).forward(types, ei, ev)
    return cfg, sd, types, ei, ev, ref, r32


def test_whole_model_both_hosts():
    """SevenNet-0's shape on smoke()'s cell at max|F| = 8 eV/A.  Forces: error against the fp64 oracle at most 1.5 x the fp32 oracle's
    own.  Energy and atomic energies bit-identical to the switch-off path (the forward pass is not touched).  Python host == native
    host bit for bit, switch on and off."""
    from sevennet_amd.engine import HipForceEngine, build_graph
    from sevennet_amd.native_model import NativeModel
    cfg, sd, types, ei, ev, ref, r32 = _smoke_cell()
    g = build_graph(types, ei, ev, device=DEV)
    n = len(types)
    f_ref, e_ref = ref['forces'].numpy(), float(ref['energy'])
    dF32 = np.abs(r32['forces'].double().numpy() - f_ref).max()
    out = {}
    for mode in (False, True):
        eng = HipForceEngine(cfg, sd, device=DEV, layer0_moments=mode)
        assert (eng.l0_plans is not None) == mode
        out[mode] = eng.compute(g)
        nat = NativeModel(cfg, sd, device=DEV, layer0_moments=mode).compute(g)
        torch.cuda.synchronize()
        for k in ('energy', 'atomic_energy', 'forces', 'dE_dr', 'virial'):
            assert torch.equal(out[mode][k], nat[k]), (mode, k)
    assert torch.equal(out[True]['energy'], out[False]['energy']) and torch.equal(out[True]['atomic_energy'], out[False]['atomic_energy'])
    assert not torch.equal(out[True]['forces'], out[False]['forces'])     # (the switch does select another reverse pass)
    for mode in (False, True):
        dF = np.abs(out[mode]['forces'].cpu().numpy() - f_ref).max()
        print(f'layer0_moments={mode}: max|dF| vs fp64 {dF:.3e} at max|F| {np.abs(f_ref).max():.3g} eV/A (fp32 oracle {dF32:.3e}, ratio {dF / dF32:.2f}); '
              f'|dE|/N {abs(float(out[mode]["energy"].cpu()) - e_ref) / n:.3e}')
    assert dF <= 1.5 * dF32, (dF, dF32)


def test_species_slots_and_a_two_system_batch():
    """mini SevenNet-0 with 3 species of which one is on no atom, and a 6-species model of which 2 occur (compact slots): two systems
    in one batch (seg_ptr), each against its fp64 oracle with the fp32-class rule relative to the switch-off engine (an error below
    one fp32 rounding of the largest force counts as that rounding), energies bit-equal to the switch-off engine, hosts bit-equal"""
    from oracle.model import OracleModel
    from sevennet_amd.batch import build_batch_graph
    from sevennet_amd.engine import HipForceEngine
    from sevennet_amd.native_model import NativeModel
    from sevennet_amd.neighbor import neighbor_list
    from sevennet_amd.shapes import mini_sevennet_0_config
    from sevennet_amd.synthetic import random_state_dict
    from helpers import three_small_systems
    for ns, remap in ((3, {0: 0, 1: 2}), (6, {0: 1, 1: 4})):
        cfg = mini_sevennet_0_config(ns)
        sd = random_state_dict(cfg, seed=ns)
        systems = [(np.vectorize(remap.get)(s[0]), s[1], s[2], s[3]) for s in three_small_systems(1)[1:]]   # 5-atom molecule, 8-atom slab
        g = build_batch_graph([s[0] for s in systems], [s[1] for s in systems], np.stack([s[2] for s in systems]),
                              np.array([s[3] for s in systems]), cfg['cutoff'], ns, device=DEV)
        assert g.seg_ptr is not None and g.n_edges > 0
        on = HipForceEngine(cfg, sd, device=DEV)
        off = HipForceEngine(cfg, sd, device=DEV, layer0_moments=False)
        a, b = on.compute(g), off.compute(g)
        nat = NativeModel(cfg, sd, device=DEV).compute(g)
        torch.cuda.synchronize()
        plans = on.l0_plans
        assert list(plans) == [tuple(range(ns))] if ns <= 4 else list(plans) == [tuple(sorted(remap.values()))]
        assert torch.equal(a['forces'], nat['forces']) and torch.equal(a['energy'], nat['energy'])
        sp = g.seg_ptr_host
        for i, (ty, pos, cell, pbc) in enumerate(systems):
            ei, ev, _ = neighbor_list(pos, cell, pbc, cfg['cutoff'])
            ref = OracleModel(cfg, sd, dtype=torch.float64).forward(ty, ei, ev)
            f_ref = ref['forces'].numpy()
            d_on = np.abs(a['forces'][sp[i]:sp[i + 1]].cpu().numpy() - f_ref).max()
            d_off = np.abs(b['forces'][sp[i]:sp[i + 1]].cpu().numpy() - f_ref).max()
            print(f'{ns} species, system {i}: max|F| {np.abs(f_ref).max():.3g}, forces vs fp64 off {d_off:.3e} on {d_on:.3e}')
            assert d_on <= 1.5 * max(d_off, 2.0 ** -23 * np.abs(f_ref).max())
        assert torch.equal(a['energy_per_system'], b['energy_per_system']) and torch.equal(a['atomic_energy'], b['atomic_energy'])
