"""GPU: the last layer's reverse pass in one source-grouped launch (snet_lastlayer_conv_bwd, csrc/snet_lastlayer.hip) against
the fp64 restatement (tests/lastlayer_ref.py) and against the pair of launches it replaces (tangent-mode reverse kernel + transposed
scalar convolution) on the same inputs, then the whole model: switch on / off, both hosts, a model file without the key."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from lastlayer_ref import hand_graph, lastlayer_reference, mixed_factors, random_inputs, without_meta_key
from test_ops_gpu import _lib, _p, _work_list

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CST_SILU = 1.6791767923989418
SCALE = 0.05
# (shape, ghost source rows): one 16-channel tile per l at lmax 1 / 2, SevenNet-0's last layer (8 / 4 / 2 tiles), an lmax-3 last layer
# (four blocks, the largest W2 image) and a shape with a source block no path reads (a dead range of g_h)
CASES = [('last16_l1', False), ('last16_l2', True), ('sevennet_0', True), ('sevennet_l3i5', False), ('last16_o3_dead', True)]


def _spec(name):
    from sevennet_amd.model_spec import build_model_spec, sevennet_0_config, sevennet_l3i5_config
    from sevennet_amd.shapes import lastlayer_test_configs
    cfgs = dict(lastlayer_test_configs(), sevennet_0=sevennet_0_config(), sevennet_l3i5=sevennet_l3i5_config())
    return build_model_spec(cfgs[name]).layers[-1].conv


@functools.lru_cache(maxsize=None)
def _problem(name, ghost):
    """graph, unit-scale inputs, real harmonics (fp32, as every kernel reads them) and the plans of both paths, built once per shape"""
    L, lib = _lib()
    spec = _spec(name)
    g = hand_graph(40, 4, seed=3, ghost_degrees=(0, 5, 16, 20)) if ghost else hand_graph(44, 0, seed=4)
    c = random_inputs(spec, g, seed=5)
    lmax, nsh, E = len(spec.paths) - 1, spec.irreps_sh.dim, g['E']
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    vec = t(g['edge_vec'])
    P = L.EdgeParams(5.0, 8, 0, 6, 0.0, lmax, 1)
    cf = (C.c_float * 8)(*[(k + 1) * np.pi / 5.0 for k in range(8)])
    emb, sh, dsh = torch.empty(E, 8, device=DEV), torch.empty(E, nsh, device=DEV), torch.empty(E, 3 * nsh, device=DEV)
    L.check(lib.snet_edge_embed_fwd(C.byref(P), cf, _p(vec), E, _p(emb), _p(sh), _p(dsh), None))
    torch.cuda.synchronize()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    plan, mplan, mlp, fplan, tconv, tmlp, tplan = (C.c_void_p() for _ in range(7))
    L.check(lib.snet_conv_plan_create(spec.tag.encode(), C.byref(plan)))
    L.check(lib.snet_lastlayer_plan_create(plan, C.c_void_p(c['W2'].ctypes.data), C.byref(mplan)), 'snet_lastlayer_plan_create')
    # today's pair: the tangent-mode reverse kernel on W2, the forward kernel of the transposed shape on W2 with its column factors
    W0, W1 = np.zeros((8, 64), np.float32), np.zeros((64, 64), np.float32)   # (the hidden layers are not run: h2 / h2' are inputs)
    wn = spec.weight_numel
    L.check(lib.snet_radial_mlp_plan_create(8, 64, 64, wn, fp(W0), fp(W1), fp(c['W2']), 0, CST_SILU, 1, C.byref(mlp)))
    L.check(lib.snet_fused_plan_create(plan, mlp, 4, C.byref(fplan)))
    ttag, col = C.create_string_buffer(13), np.empty(wn, np.float32)
    dead, nd = (C.c_int32 * 32)(), C.c_int32()
    L.check(lib.snet_conv_plan_transposed(plan, ttag, col.ctypes.data_as(C.c_void_p), C.cast(dead, C.c_void_p), 32, C.byref(nd)))
    w2t = np.ascontiguousarray(c['W2'] * col[None, :], dtype=np.float32)
    L.check(lib.snet_conv_plan_create(ttag.value, C.byref(tconv)))
    L.check(lib.snet_radial_mlp_plan_create(8, 64, 64, wn, fp(W0), fp(W1), fp(w2t), 0, CST_SILU, 1, C.byref(tmlp)))
    L.check(lib.snet_fused_plan_create(tconv, tmlp, 4, C.byref(tplan)))
    return dict(spec=spec, g=g, c=c, sh=sh, dsh=dsh, vec=vec, mplan=mplan, fplan=fplan, tplan=tplan, n_dead=nd.value,
                keep=(plan, mlp, tconv, tmlp))   # (plans live as long as the cache)


def _run(name, ghost, mixed):
    """-> dict of fp64 arrays: g_h / g_vec of the new entry point and of today's pair, the fp64 restatement, and the new path's raw
    device outputs (for the bit comparisons)"""
    L, lib = _lib()
    pr = _problem(name, ghost)
    spec, g, c = pr['spec'], pr['g'], pr['c']
    N, NT, E, dx = g['N'], g['NT'], g['E'], spec.irreps_x.dim
    x, g_out, h2, h2d = c['x'], c['g_out'], c['h2'], c['h2d']
    if mixed:
        fg, fh, fhd = mixed_factors(g, len(h2))
        g_out, h2, h2d = g_out * fg[:, None], h2 * fh[:, None], h2d * fhd[:, None]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    X, G, H2, H2D, wr = t(x), t(g_out), t(h2), t(h2d), t(c['w_row'])
    rp, src, cp, ep, ct = t(g['row_ptr']), t(g['src']), t(g['col_ptr']), t(g['eperm']), t(g['center_t'])
    wrt = wr[ep.long()].contiguous()
    sh, dsh, vec = pr['sh'], pr['dsh'], pr['vec']
    zero = torch.zeros(E, 3, device=DEV)

    def new(ranges, prior=zero):
        gh = torch.full((NT + 1, dx), float('nan'), device=DEV)
        gv = torch.cat([prior, torch.zeros(1, 3, device=DEV)])
        for a, b in ranges:
            L.check(lib.snet_lastlayer_conv_bwd(pr['mplan'], _p(X), _p(G), _p(sh), _p(dsh), _p(vec), _p(H2), _p(H2D), _p(cp), _p(ct), _p(wrt),
                                                _p(ep), a, b, SCALE, _p(gh), _p(gv), None), 'snet_lastlayer_conv_bwd')
        torch.cuda.synchronize()
        assert torch.isnan(gh[NT]).all() and (gv[E] == 0).all()        # nothing beyond the rows / edges of the call
        return gh[:NT], gv[:E]

    gh_new, gv_new = new([(0, NT)])
    # ---- today's pair on the same inputs
    gv_old, gh_old = torch.zeros(E, 3, device=DEV), torch.zeros(NT, dx, device=DEV)
    tile_ptr, tile_node, n_tiles = _work_list(L, lib, pr['fplan'], rp, torch.from_numpy(g['row_ptr']), N, E, DEV)
    x_max, g_max = torch.empty(NT, device=DEV), torch.empty(N, device=DEV)
    L.check(lib.snet_row_absmax(_p(X), NT, dx, _p(x_max), None))
    L.check(lib.snet_row_absmax(_p(G), N, spec.irreps_out.dim, _p(g_max), None))
    L.check(lib.snet_conv_bwd_fused_tangent(pr['fplan'], _p(X), _p(sh), _p(dsh), _p(H2), _p(H2D), _p(wr), _p(rp), _p(src), _p(tile_ptr),
                                            _p(tile_node), n_tiles.value, SCALE, _p(G), None, _p(vec), _p(gv_old), _p(x_max), _p(g_max), None))
    sh_t = sh[ep.long()].contiguous()
    L.check(lib.snet_conv_fwd_fused(pr['tplan'], _p(G), _p(sh_t), _p(H2), _p(wrt), _p(cp), _p(ct), NT, SCALE, _p(gh_old), None))
    torch.cuda.synchronize()
    T = torch.from_numpy
    ref_h, ref_v = lastlayer_reference(spec, T(x), T(g_out), sh.cpu(), dsh.cpu(), T(g['edge_vec']), T(h2), T(h2d), T(c['W2']), T(c['w_row']),
                                       T(g['row_ptr']), T(g['src']), SCALE)
    f64 = lambda a: a.double().cpu().numpy()  # noqa: E731
    return dict(gh_new=f64(gh_new), gv_new=f64(gv_new), gh_old=f64(gh_old), gv_old=f64(gv_old), ref_h=ref_h.numpy(),
                ref_v=ref_v.numpy(), raw=(gh_new, gv_new), new=new, N=N, NT=NT, n_dead=pr['n_dead'])


@pytest.mark.parametrize('mixed', [False, True], ids=['unit', 'mixed'])
@pytest.mark.parametrize('name,ghost', CASES)
def test_entry_point_vs_fp64_and_todays_pair(name, ghost, mixed):
    """g_h and g_vec against the fp64 restatement; the project's fp32-class rule (tests/test_tangent_gpu.py, test_layer0_moments_gpu.py):
    per output, the new path's error is at most 1.5 x the error of today's pair of launches on the same inputs.  Source out-degrees
    0, 1, 15, 16, 17, 32, 33, 49; g_h is NaN on entry and must be written whole, dead ranges as zeros.  mixed: g_out rows spanning 2^+-20, h2 / h2' rows scaled by powers of two across a tile, one all-zero h2 row."""
    r = _run(name, ghost, mixed)
    assert np.isfinite(r['gh_new']).all() and np.isfinite(r['gv_new']).all()
    assert (r['n_dead'] > 0) == (name == 'last16_o3_dead')
    for out, new, old, ref in (('g_h', r['gh_new'], r['gh_old'], r['ref_h']), ('g_vec', r['gv_new'], r['gv_old'], r['ref_v'])):
        e_new, e_old = np.abs(new - ref).max(), np.abs(old - ref).max()
        print(f'lastlayer {name} ghost={ghost} {"mixed" if mixed else "unit"} {out}: max|ref| {np.abs(ref).max():.3g}, error vs fp64 '
              f'pair {e_old:.3e} merged {e_new:.3e}, ratio {e_new / e_old:.2f}')
        assert e_new <= 1.5 * e_old, (out, e_new, e_old)


@pytest.mark.parametrize('name,ghost', [('last16_l2', True), ('sevennet_0', True)])
def test_same_bits_twice_and_over_split_ranges(name, ghost):
    """two launches on the same inputs give the same bits; ghost rows [N, NT) first and [0, N) later (the order of both hosts' halo
    split) give the bits of one call over [0, NT)"""
    r = _run(name, ghost, False)
    gh, gv = r['raw']
    gh2, gv2 = r['new']([(0, r['NT'])])
    assert torch.equal(gh, gh2) and torch.equal(gv, gv2)
    gh3, gv3 = r['new']([(r['N'], r['NT']), (0, r['N'])])
    assert torch.equal(gh, gh3) and torch.equal(gv, gv3)
    assert r['NT'] > r['N']
    # g_vec is ADDED to: a launch onto a nonzero prior value gives fl(prior + its own contribution), the contribution being what a
    # launch onto zeros leaves (one fp32 addition per entry, the same one torch performs)
    prior = torch.from_numpy(np.random.default_rng(9).normal(0, 1, tuple(gv.shape)).astype(np.float32)).to(DEV)
    gh4, gv4 = r['new']([(0, r['NT'])], prior)
    assert torch.equal(gh, gh4) and torch.equal(gv4, prior + gv) and not torch.equal(gv4, gv)


def test_plan_refuses_shapes_outside_its_domain():
    from sevennet_amd.model_spec import build_model_spec, sevennet_0_config
    L, lib = _lib()
    layers = build_model_spec(sevennet_0_config()).layers
    W2 = np.zeros((64, 4096), np.float32)
    for ls in (layers[0], layers[2]):       # outputs of every l: no transposed scalar product
        plan, mp = C.c_void_p(), C.c_void_p()
        L.check(lib.snet_conv_plan_create(ls.conv.tag.encode(), C.byref(plan)))
        assert lib.snet_lastlayer_plan_create(plan, C.c_void_p(W2.ctypes.data), C.byref(mp)) != 0
        assert not mp.value and b'snet_lastlayer_plan_create' in lib.snet_last_error()
        lib.snet_conv_plan_destroy(plan)
    assert lib.snet_lastlayer_conv_bwd(None, *([None] * 11), 0, 1, 1.0, None, None, None) != 0               # null plan: refused, not run


def test_whole_model_switch_hosts_and_old_files(tmp_path):
    """SevenNet-0's shape on smoke()'s cell at max|F| = 8 eV/A.  Forces: error against the fp64 oracle with the switch on at most
    1.5 x that with it off; energy and atomic energies bit-identical (the forward pass is untouched).  Python host == native host
    bit for bit with the switch on.  A .snet file without the key runs the pair of launches."""
    from sevennet_amd.engine import HipForceEngine, build_graph
    from sevennet_amd.model_file import write_model_file
    from sevennet_amd.native_model import NativeModel
    from test_layer0_moments_gpu import _smoke_cell
    cfg, sd, types, ei, ev, ref, _ = _smoke_cell()
    g = build_graph(types, ei, ev, device=DEV)
    f_ref = ref['forces'].numpy()
    out, dF = {}, {}
    for mode in (False, True):
        eng = HipForceEngine(cfg, sd, device=DEV, last_layer_merged=mode)
        assert (eng.layers[-1].mplan is not None) == mode and all(L_.mplan is None for L_ in eng.layers[:-1])
        out[mode] = eng.compute(g)
        torch.cuda.synchronize()
        dF[mode] = np.abs(out[mode]['forces'].cpu().numpy() - f_ref).max()
        print(f'lastlayer whole model last_layer_merged={mode}: max|dF| vs fp64 {dF[mode]:.3e} at max|F| {np.abs(f_ref).max():.3g} eV/A')
    print(f'lastlayer whole model: ratio on / off {dF[True] / dF[False]:.2f}, max|F_on - F_off| '
          f'{(out[True]["forces"] - out[False]["forces"]).abs().max().item():.3e}')
    assert torch.equal(out[True]['energy'], out[False]['energy']) and torch.equal(out[True]['atomic_energy'], out[False]['atomic_energy'])
    assert not torch.equal(out[True]['forces'], out[False]['forces'])     # (the switch does select another reverse pass)
    assert dF[True] <= 1.5 * dF[False], dF
    nat = {mode: NativeModel(cfg, sd, device=DEV, last_layer_merged=mode).compute(g) for mode in (False, True)}
    torch.cuda.synchronize()
    for mode in (False, True):
        for k in ('energy', 'atomic_energy', 'forces', 'dE_dr', 'virial'):
            assert torch.equal(out[mode][k], nat[mode][k]), (mode, k)
    path, old = tmp_path / 'new.snet', tmp_path / 'old.snet'
    write_model_file(str(path), cfg, sd)
    old.write_bytes(without_meta_key(path.read_bytes(), 'last_layer_merged'))
    a, b = NativeModel(str(path), device=DEV).compute(g), NativeModel(str(old), device=DEV).compute(g)
    torch.cuda.synchronize()
    assert torch.equal(a['forces'], out[True]['forces']) and torch.equal(b['forces'], out[False]['forces'])
